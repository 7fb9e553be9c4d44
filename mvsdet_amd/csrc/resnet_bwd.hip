// Gradients of one ResNet bottleneck with frozen BatchNorm (resnet.hip has the forward and the definition).  With W' = scale (.) W,
//   a = relu(W1' x + t1),  b = relu(conv3x3_s(a; W2') + t2),  out = relu(W3' b + t3 + id),  id = x | Wd' x[.., s y, s x] + td
// and g = dL/dout given:
//
//   gz  = gate(g, out)                                    resnet_relu_gate_kernel
//   dW3 = scale3 (.) (gz b^T)                             fpn_dw_kernel<1> (fpn_bwd.hip); the rows' scale is the caller's
//   gb  = gate(W3'^T gz, b)                               resnet_dx1x1_kernel
//   dW2 = scale2 (.) dw3x3_s(gb, a)                       s = 1: fpn_dw_kernel<9>;  s = 2: resnet_dw_s2_kernel<9>
//   ga  = gate(convT3x3_s(gb; W2'), a)                    s = 1: resnet_dx3x3_s1_kernel;  s = 2: resnet_dx3x3_s2_kernel, four classes
//   dW1 = scale1 (.) (ga x^T)                             fpn_dw_kernel<1>
//   dx  = (W1'^T ga) + ( gz | spread_s(Wd'^T gz) )        resnet_dx1x1_kernel, twice with the downsample branch; spread_s puts (yo, xo)
//                                                         at (s yo, s xo), zero elsewhere
//   dWd = scaled (.) (gz x[.., s y, s x]^T)               s = 1: fpn_dw_kernel<1>;  s = 2: resnet_dw_s2_kernel<1>
//
// The gate, once: gate(v, y) = y <= 0 ? 0 : v on the SAVED OUTPUT y of the ReLU.  That is ATen's threshold_backward, the gradient rule of
// torch.relu: the gradient is dropped (a +0.0, whatever v holds, a NaN included) where y is 0.0, -0.0 or negative, and passes where y is
// positive, +inf or NaN (NaN <= 0 is false).  tests/test_resnet_grad_host.py pins the table against torch on the CPU.
//
// The order of the additions inside dx is fixed: the GEMM's accumulator first, then + the residual (gz, or the half-resolution
// Wd'^T gz where y and x are both even; no addition elsewhere), then the gate where a gate map is given.
//
// resnet_dx1x1_kernel: resnet_conv1x1_kernel's GEMM (gemm_bf16x3_block, 128 rows x 64 columns) on the split of W'^T: the rows are the
//   layer's INPUT channels, zero-padded to a multiple of 128 as in the forward; the columns run over all views' pixels.
// resnet_dx3x3_s1_kernel: the forward 3x3 loop (resnet_conv3x3.h) on the flipped, transposed weight w'[c,o,dy,dx] = W'[o,c,2-dy,2-dx].
// resnet_dx3x3_s2_kernel: the transposed convolution of stride 2 WITHOUT the inserted zeros.  Input pixel (y, x) receives the taps with
//   y + 1 - dy and x + 1 - dx even: an even coordinate takes dy = 1 from output pixel y / 2; an odd one takes dy = 0 from (y + 1) / 2 and
//   dy = 2 from (y - 1) / 2.  So the map falls into four parity classes (py, px) of (1 + py)(1 + px) = 1, 2, 2, 4 taps, 2.25 a pixel on
//   average against 9.  One launch per class: gemm_bf16x3_block with K = (taps of the class) x Cout, tap-major in the order (dy ascending,
//   dx ascending); the fetch reads the class's half-resolution pixel (i + [py and dy = 0], j + [px and dx = 0]) of gb, or zero at or
//   beyond (Ho, Wo); the store scatters to (2 i + py, 2 j + px).  The four split matrices lie behind one another in `wsplit`.  Any H, W:
//   Ho = (H - 1) / 2 + 1, and the last odd row or column may have no partner beyond it (its dy = 0 tap reads zero).
// resnet_dw_s2_kernel<TAPS>: the weight gradient of a stride-2 convolution, the contract of fpn_dw_kernel: a GEMM whose reduction index is
//   the OUTPUT pixel, D[o][c] += gy[o][k] x[k][c] per tap on v_mfma_f32_32x32x16_bf16, bf16x3 with the small products first.  Only the
//   real multiply-adds: no space-to-depth detour.
//     block = 128 output channels x 32 input channels x all taps; wave w owns rows 32 w .. 32 w + 31 and TAPS accumulators.
//     tile  = 2 x 16 output pixels of gy and, for nine taps, the 5 x 33 halo of x kept per row as EVEN halo columns (17) then ODD ones (16):
//             halo column 2 lx + dx is the even lx (dx = 0), the odd lx (dx = 1) or the even lx + 1 (dx = 2), so a fragment's eight
//             pixels are eight consecutive bf16: one ds_read_b128 for dx = 0 and dx = 1, the dx = 2 fragment formed from the dx = 0 one and
//             the next pair with v_alignbit_b32.  One tap: the 2 x 16 pixels (2 yo, 2 xo) alone.
//     stage = one LDS stage (47 KiB | 25 KiB), the next tile in registers under this tile's MFMAs, two barriers a tile.  Padding and the
//             ragged edge read a zero word: the ADDRESS is selected, nothing outside the two maps is read.
//     K     = the tiles (view-major) are dealt to `nsplit` blocks in contiguous runs; every split writes its fp32 partial
//             [split][tap][o][c] to the workspace and resnet_dw_s2_sum_kernel adds the splits in ascending order (dw_sum.h).
//
// No atomics anywhere: the same bits on every run.  Element offsets are 64-bit.
#include "common.h"
#include "dw_sum.h"
#include "mfma.h"
#include "resnet_conv3x3.h"

namespace mvsdet {

// the gradient rule of torch.relu on the saved output y (the header has the table)
__device__ __forceinline__ float rn_gate(float v, float y) { return y <= 0.0f ? 0.0f : v; }

__global__ __launch_bounds__(kThreads) void resnet_relu_gate_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                                    float* __restrict__ out, long long total) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e < total) out[e] = rn_gate(g[e], y[e]);
}

// g (N,K,H,W), out and gate_map (N,M,H,W); residual (N,M,H,W) (spread = 1) or (N,M,Hr,Wr) read at (y / 2, x / 2) where both are even
// (spread = 2); columns v = n HW + pixel, V = N HW of them
__global__ __launch_bounds__(kThreads) void resnet_dx1x1_kernel(const float* __restrict__ g, const uint4* __restrict__ ws,
                                                                const float* __restrict__ residual, const float* __restrict__ gate_map,
                                                                float* __restrict__ out, int M, int K, int HW, int W, int V, int spread,
                                                                int HWr, int Wr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.y * kGemmBM, v0 = blockIdx.x * kGemmBN;

    // staging duty: column v0 + (tid & 63), channels 8 * (tid >> 6) .. + 7 of the step
    const int sv = v0 + (tid & 63), skq = tid >> 6;
    const bool sv_ok = sv < V;
    const int sn = sv_ok ? sv / HW : 0, spix = sv_ok ? sv - sn * HW : 0;
    const float* gs = g + ((size_t)sn * K + 8 * skq) * HW + spix;
    float f[8];
    auto fetch = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = sv_ok ? gs[(size_t)(ks * kGemmBK + j) * HW] : 0.0f;
    };

    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.0f;
    gemm_bf16x3_block(acc, f, fetch, ws, m0, K, tid, wave);

    // ---- epilogue: acc [+ residual], then the gate
    const int mw = m0 + 32 * wave;
    if (mw >= M) return;                                   // rows of the zero padding: nothing to store (after the last barrier)
    const int half = lane >> 5;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int v = v0 + 32 * c + (lane & 31);
        if (v >= V) continue;
        const int n = v / HW, pix = v - n * HW;
        const size_t base = ((size_t)n * M + mw) * HW + pix;
        const int y = pix / W, x = pix - y * W;
        const bool at_even = !((y | x) & 1);
        const size_t rbase = ((size_t)n * M + mw) * HWr + (size_t)(y >> 1) * Wr + (x >> 1);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mfma32_row(i, half);
            const size_t o = base + (size_t)row * HW;
            float val = acc[c][i];
            if (residual) {
                if (spread == 1) val += residual[o];
                else if (at_even) val += residual[rbase + (size_t)row * HWr];
            }
            if (gate_map) val = rn_gate(val, gate_map[o]);
            out[o] = val;
        }
    }
}

// g (N,K,H,W), ws = split (ceil128(M), 9 K) tap-major matrix of the flipped, transposed weight, out and gate_map (N,M,H,W)
__global__ __launch_bounds__(kThreads) void resnet_dx3x3_s1_kernel(const float* __restrict__ g, const uint4* __restrict__ ws,
                                                                   const float* __restrict__ gate_map, float* __restrict__ out, int M, int K,
                                                                   int H, int W, int tiles_x) {
    using T = RnTile<1>;
    const size_t HW = (size_t)H * W;
    rn_conv3x3_block<1>(g, ws, M, K, H, W, tiles_x, [&](const f32x16 (&acc)[T::NT], int n, int mw, int y0, int x0, int lx, int ly, int half) {
#pragma unroll
        for (int t = 0; t < T::NT; ++t) {
            const int y = y0 + 2 * t + ly, xx = x0 + lx;
            if (y >= H || xx >= W) continue;
            const size_t o = ((size_t)n * M + mw) * HW + (size_t)y * W + xx;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const size_t e = o + (size_t)mfma32_row(i, half) * HW;
                out[e] = gate_map ? rn_gate(acc[t][i], gate_map[e]) : acc[t][i];
            }
        }
    });
}

// One parity class (py, px) of the stride-2 transposed 3x3: gb (N,K,Ho,Wo), ws = the class's split (ceil128(M), nty ntx K) matrix, out and
// gate_map (N,M,H,W); the class's pixels (2 i + py, 2 j + px), i < Hc, j < Wc; columns v = (n Hc + i) Wc + j, V of them
__global__ __launch_bounds__(kThreads) void resnet_dx3x3_s2_kernel(const float* __restrict__ gb, const uint4* __restrict__ ws,
                                                                   const float* __restrict__ gate_map, float* __restrict__ out, int M, int K,
                                                                   int H, int W, int Ho, int Wo, int py, int px, int Hc, int Wc, int V) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.y * kGemmBM, v0 = blockIdx.x * kGemmBN;
    const int HWc = Hc * Wc, ntx = 1 + px, spt = K / kGemmBK;   // K steps per tap
    const size_t HWo = (size_t)Ho * Wo;

    const int sv = v0 + (tid & 63), skq = tid >> 6;
    const bool sv_ok = sv < V;
    const int sn = sv_ok ? sv / HWc : 0, srem = sv_ok ? sv - sn * HWc : 0;
    const int si = srem / Wc, sj = srem - si * Wc;
    const float* gs = gb + ((size_t)sn * K + 8 * skq) * HWo;
    float f[8];
    auto fetch = [&](int ks) {
        const int t = ks / spt, a = t / ntx, b = t - a * ntx;   // the class's tap (a, b): dy = py ? 2 a : 1, dx = px ? 2 b : 1
        const int yo = si + ((py != 0) & (a == 0)), xo = sj + ((px != 0) & (b == 0));
        const bool ok = sv_ok & (yo < Ho) & (xo < Wo);
        const float* p = gs + (size_t)((ks - t * spt) * kGemmBK) * HWo + (ok ? (size_t)yo * Wo + xo : 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = ok ? p[(size_t)j * HWo] : 0.0f;
    };

    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.0f;
    gemm_bf16x3_block(acc, f, fetch, ws, m0, (1 + py) * ntx * K, tid, wave);

    const int mw = m0 + 32 * wave;
    if (mw >= M) return;
    const int half = lane >> 5;
    const size_t HW = (size_t)H * W;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int v = v0 + 32 * c + (lane & 31);
        if (v >= V) continue;
        const int n = v / HWc, rem = v - n * HWc, i0 = rem / Wc, j0 = rem - i0 * Wc;
        const size_t base = ((size_t)n * M + mw) * HW + (size_t)(2 * i0 + py) * W + (2 * j0 + px);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const size_t e = base + (size_t)mfma32_row(i, half) * HW;
            out[e] = gate_map ? rn_gate(acc[c][i], gate_map[e]) : acc[c][i];
        }
    }
}

// ------------------------------------------------------------------------------------------- the stride-2 weight gradient
constexpr int kD2TH = 2, kD2TW = 16;                  // OUTPUT pixels of a tile
constexpr int kD2BM = 128, kD2BC = 32;                // output x input channels of a block
constexpr int kD2SplitBlocks = 512;                   // K is split until about this many blocks run (two per CU)
constexpr int kD2MaxSplit = 65535;
constexpr int kD2GyChanB = kD2TH * 32 + 16;           // 80 B: 5 units
constexpr int kD2GyPieceB = kD2BM * kD2GyChanB;       // 10240
constexpr int kD2GyPerRound = kThreads / (2 * kD2TH); // 64 output channels of gy per staging round
constexpr int kD2GyRounds = kD2BM / kD2GyPerRound;    // 2

template <int TAPS> struct Dw2Shape {
    static constexpr int kXRows = TAPS == 9 ? 2 * (kD2TH - 1) + 3 : kD2TH;      // 5 halo rows | the 2 rows 2 yo
    static constexpr int kEvenB = TAPS == 9 ? 48 : 0;                            // 17 even halo columns (+ pad) in front of the 16 odd ones
    static constexpr int kXRowB = kEvenB + 32;                                   // 80 | 32
    static constexpr int kXChanB = TAPS == 9 ? kXRows * kXRowB + 32 : kXRows * kXRowB + 16;   // 432 B = 27 units | 80 B = 5 units: odd
    static constexpr int kXPieceB = kD2BC * kXChanB;                             // 13824 | 2560
    static constexpr int kXUnits = kD2BC * kXRows * 4;                           // (channel, row, q): 8 halo columns | 4 pixels each: 640 | 256
    static constexpr int kXRounds = (kXUnits + kThreads - 1) / kThreads;         // 3 | 1
    static constexpr int kEdgeUnits = TAPS == 9 ? kD2BC * kXRows : 0;            // (channel, row): halo column 32, the 17th even one: 160
    static_assert(kEdgeUnits <= kThreads, "one thread per edge pixel");
};

__device__ float4 g_rnb_zero;   // zero-initialised: the source of every padding element

// gy (N,Cout,Ho,Wo), x (N,C,H,W), partial [nsplit][TAPS][Cout][C]; grid (C/32, Cout/128, nsplit)
template <int TAPS>
__global__ __launch_bounds__(kThreads, 2) void resnet_dw_s2_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                   float* __restrict__ partial, int C, int Cout, int H, int W, int Ho, int Wo,
                                                                   int tiles_x, int tiles_y, int ntiles, int per_split) {
    using S = Dw2Shape<TAPS>;
    __shared__ __attribute__((aligned(16))) char s_gy[2 * kD2GyPieceB];
    __shared__ __attribute__((aligned(16))) char s_x[2 * S::kXPieceB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = blockIdx.x * kD2BC, o0 = blockIdx.y * kD2BM, split = blockIdx.z;
    const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
    const float* const zero = reinterpret_cast<const float*>(&g_rnb_zero);

    // ---- staging roles, the same for every tile: gy unit (channel go + 64 a, row grow, half gh)
    const int gh = tid & 1, grow = (tid >> 1) & (kD2TH - 1), go = tid / (2 * kD2TH);
    const int g_lds = go * kD2GyChanB + grow * 32 + gh * 16;
    const float* const gchan = gy + (size_t)(o0 + go) * HWo;
    // X unit u = tid + kThreads a -> (channel u / (4 rows), row, q = u & 3), worked out where it is used: kept, the roles cost the
    // registers that the nine accumulators need
    auto x_role = [&](int a, int& xc, int& xrow, int& xq) {
        const int u = min(tid + kThreads * a, S::kXUnits - 1), cr = u >> 2;
        xq = u & 3;
        xc = cr / S::kXRows;
        xrow = cr - xc * S::kXRows;
    };
    const int el = min(tid, max(S::kEdgeUnits, 1) - 1), ec = el / S::kXRows, erow = el - ec * S::kXRows;

    float fg[kD2GyRounds][8], fx[S::kXRounds][TAPS == 9 ? 8 : 4], fe;
    // the tile (n, ty, tx): its values into registers
    auto fetch = [&](int n, int ty, int tx) {
        {
            const float* gv = gchan + (size_t)n * Cout * HWo;
            const int yo = ty * kD2TH + grow, xs = tx * kD2TW + 8 * gh;
            const int cnt = yo < Ho ? Wo - xs : 0;
            const long long row = yo < Ho ? (long long)yo * Wo : 0;   // offsets stay integers until an element inside the map is chosen
#pragma unroll
            for (int a = 0; a < kD2GyRounds; ++a) {
                const float* p = gv + (size_t)(kD2GyPerRound * a) * HWo + row;
#pragma unroll
                for (int j = 0; j < 8; ++j) fg[a][j] = *(j < cnt ? p + (xs + j) : zero);
            }
        }
        const float* xv = x + ((size_t)n * C + c0) * HW;
#pragma unroll
        for (int a = 0; a < S::kXRounds; ++a) {
            int xc, xrow, xq;
            x_role(a, xc, xrow, xq);
            const bool unit_ok = tid + kThreads * a < S::kXUnits;
            if (TAPS == 9) {
                // halo row xrow of the tile, halo columns 8 q .. 8 q + 7
                const int y = 2 * ty * kD2TH - 1 + xrow, xs = 2 * tx * kD2TW - 1 + 8 * xq;
                const bool row_ok = unit_ok & (y >= 0) & (y < H);
                const float* p = xv + (size_t)xc * HW + (row_ok ? (long long)y * W : 0);
#pragma unroll
                for (int j = 0; j < 8; ++j) fx[a][j] = *((row_ok & (xs + j >= 0) & (xs + j < W)) ? p + (xs + j) : zero);
            } else {
                // pixels (2 yo, 2 xo), xo = 16 tx + 4 q .. + 3
                const int y = 2 * (ty * kD2TH + xrow), xs = 2 * (tx * kD2TW + 4 * xq);
                const bool row_ok = unit_ok & (y < H);
                const float* p = xv + (size_t)xc * HW + (row_ok ? (long long)y * W : 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) fx[a][j] = *((row_ok & (xs + 2 * j < W)) ? p + (xs + 2 * j) : zero);
            }
        }
        if (TAPS == 9) {
            const int y = 2 * ty * kD2TH - 1 + erow, xe = 2 * tx * kD2TW + 2 * kD2TW - 1;   // halo column 32
            const bool ok = (tid < S::kEdgeUnits) & (y >= 0) & (y < H) & (xe < W);
            fe = *(ok ? xv + (size_t)ec * HW + (ok ? (long long)y * W + xe : 0) : zero);
        }
    };
    // registers -> bf16 pieces in the LDS.  The values pass through an opaque statement first (fpn_bwd.hip: without it the compiler cuts
    // right behind the loads and waits for them in front of the MFMAs they were to hide under).
    auto put = [&]() {
#pragma unroll
        for (int a = 0; a < kD2GyRounds; ++a) {
            u32x4 hi, mid;
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(fg[a][j]));
            bf16x3_cut8(fg[a], hi, mid);
            char* d = s_gy + g_lds + kD2GyPerRound * a * kD2GyChanB;
            *reinterpret_cast<uint4*>(d) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            *reinterpret_cast<uint4*>(d + kD2GyPieceB) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
        }
#pragma unroll
        for (int a = 0; a < S::kXRounds; ++a) {
#pragma unroll
            for (int j = 0; j < (TAPS == 9 ? 8 : 4); ++j) asm volatile("" : "+v"(fx[a][j]));
            if (tid + kThreads * a >= S::kXUnits) continue;
            int xc, xrow, xq;
            x_role(a, xc, xrow, xq);
            char* d = s_x + xc * S::kXChanB + xrow * S::kXRowB + 8 * xq;
            unsigned h0, m0, h1, m1;
            if (TAPS == 9) {
                // even halo columns 8 q + 0, 2, 4, 6 -> even pixels 4 q .. 4 q + 3; odd ones 8 q + 1, 3, 5, 7 -> odd pixels 4 q .. 4 q + 3
                bf16x3_split2(fx[a][0], fx[a][2], h0, m0);
                bf16x3_split2(fx[a][4], fx[a][6], h1, m1);
                *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + S::kXPieceB) = make_uint2(m0, m1);
                bf16x3_split2(fx[a][1], fx[a][3], h0, m0);
                bf16x3_split2(fx[a][5], fx[a][7], h1, m1);
                *reinterpret_cast<uint2*>(d + S::kEvenB) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + S::kEvenB + S::kXPieceB) = make_uint2(m0, m1);
            } else {
                bf16x3_split2(fx[a][0], fx[a][1], h0, m0);
                bf16x3_split2(fx[a][2], fx[a][3], h1, m1);
                *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + S::kXPieceB) = make_uint2(m0, m1);
            }
        }
        if (TAPS == 9) {
            asm volatile("" : "+v"(fe));
            unsigned h0, m0;
            bf16x3_split2(fe, 0.0f, h0, m0);              // (even pixel 16, 17: never read)
            if (tid < S::kEdgeUnits) {
                char* d = s_x + ec * S::kXChanB + erow * S::kXRowB + 32;
                *reinterpret_cast<unsigned*>(d) = h0;
                *reinterpret_cast<unsigned*>(d + S::kXPieceB) = m0;
            }
        }
    };

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    const int r32 = lane & 31, hh = lane >> 5;
    const char* const ya = s_gy + (32 * wave + r32) * kD2GyChanB + hh * 16;
    const char* const xa = s_x + r32 * S::kXChanB + hh * 16;

    // the split's run of tiles, view-major; the position advances without a division
    const int t_begin = min(split * per_split, ntiles), t_end = min(t_begin + per_split, ntiles);
    const int tpv = tiles_x * tiles_y;
    int n = t_begin / tpv, ty, tx;
    {
        const int rem = t_begin - n * tpv;
        ty = rem / tiles_x;
        tx = rem - ty * tiles_x;
    }
    if (t_begin < t_end) fetch(n, ty, tx);
    for (int t = t_begin; t < t_end; ++t) {
        put();
        __syncthreads();
        if (++tx == tiles_x) {
            tx = 0;
            if (++ty == tiles_y) {
                ty = 0;
                ++n;
            }
        }
        if (t + 1 < t_end) fetch(n, ty, tx);               // in flight under the MFMAs below
#pragma unroll
        for (int r = 0; r < kD2TH; ++r) {
            const bf16x8 Ah = *reinterpret_cast<const bf16x8*>(ya + r * 32);
            const bf16x8 Am = *reinterpret_cast<const bf16x8*>(ya + kD2GyPieceB + r * 32);
            if (TAPS == 9) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    // the mid pieces of X first (hi mid), then its hi pieces (mid hi, hi hi): per accumulator the two small products before
                    // the large one
#pragma unroll
                    for (int p = 1; p >= 0; --p) {
                        const char* rowp = xa + p * S::kXPieceB + (2 * r + dy) * S::kXRowB;
                        const u32x4 ev = *reinterpret_cast<const u32x4*>(rowp);                      // even pixels 8 hh .. 8 hh + 7
                        const unsigned nxt = *reinterpret_cast<const unsigned*>(rowp + 16);          // even pixels 8 hh + 8, + 9
                        const u32x4 od = *reinterpret_cast<const u32x4*>(rowp + S::kEvenB);          // odd pixels 8 hh .. 8 hh + 7
                        bf16x8 bq[3];
                        bq[0] = __builtin_bit_cast(bf16x8, ev);                                                        // column 2 lx
                        bq[1] = __builtin_bit_cast(bf16x8, od);                                                        // column 2 lx + 1
                        bq[2] = __builtin_bit_cast(bf16x8, (u32x4{__builtin_amdgcn_alignbit(ev[1], ev[0], 16), __builtin_amdgcn_alignbit(ev[2], ev[1], 16),
                                                                  __builtin_amdgcn_alignbit(ev[3], ev[2], 16), __builtin_amdgcn_alignbit(nxt, ev[3], 16)}));   // 2 lx + 2
                        if (p == 0) {
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) acc[(3 * dy + dx) % TAPS] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, bq[dx], acc[(3 * dy + dx) % TAPS], 0, 0, 0);
                        }
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) acc[(3 * dy + dx) % TAPS] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, bq[dx], acc[(3 * dy + dx) % TAPS], 0, 0, 0);
                    }
                }
            } else {
                const char* rowp = xa + r * S::kXRowB;
                bf16x3_mfma32(acc[0], Ah, Am, *reinterpret_cast<const bf16x8*>(rowp), *reinterpret_cast<const bf16x8*>(rowp + S::kXPieceB));
            }
        }
        __syncthreads();                                   // the stage is free for the next tile's pieces
    }

    // partial[split][tap][o][c]: column = lane & 31 (c), row = mfma32_row (o): 128-byte runs
    float* pw = partial + (((size_t)split * TAPS) * Cout + o0 + 32 * wave) * C + c0 + r32;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) pw[((size_t)t * Cout + mfma32_row(i, hh)) * C] = acc[t][i];
}

__global__ __launch_bounds__(kThreads) void resnet_dw_s2_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw, int nsplit, int taps,
                                                                    long long oc) {
    dw_sum_splits(partial, dw, nsplit, taps, oc);
}

struct Dw2Plan {
    int Ho, Wo, tiles_x, tiles_y, nsplit, per_split;
    long long ntiles;
};

// host only: the tiles and the split of K.  false: the shape is refused (the message is set)
static bool dw2_plan(const char* who, int taps, int N, int C, int Cout, int H, int W, Dw2Plan& p) {
    if (taps != 1 && taps != 9) {
        set_error("%s: taps=%d must be 1 or 9", who, taps);
        return false;
    }
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0) {
        set_error("%s: bad shape N=%d H=%d W=%d (1 <= N <= 65535)", who, N, H, W);
        return false;
    }
    if (C <= 0 || C % kD2BC || Cout <= 0 || Cout % kD2BM || Cout / kD2BM > 65535 || C / kD2BC > INT32_MAX / 2) {
        set_error("%s: C=%d must be a multiple of %d and Cout=%d of %d", who, C, kD2BC, Cout, kD2BM);
        return false;
    }
    if ((long long)H * W >= INT32_MAX) {
        set_error("%s: map %d x %d too large", who, H, W);
        return false;
    }
    p.Ho = (H - 1) / 2 + 1;
    p.Wo = (W - 1) / 2 + 1;
    if ((long long)N * p.Ho * p.Wo >= INT32_MAX) {
        set_error("%s: N Ho Wo = %lld columns exceed 2^31", who, (long long)N * p.Ho * p.Wo);
        return false;
    }
    p.tiles_x = (p.Wo + kD2TW - 1) / kD2TW;
    p.tiles_y = (p.Ho + kD2TH - 1) / kD2TH;
    p.ntiles = (long long)N * p.tiles_x * p.tiles_y;
    const long long per_k = (long long)(C / kD2BC) * (Cout / kD2BM);
    long long want = (kD2SplitBlocks + per_k - 1) / per_k;
    want = want < 1 ? 1 : want;
    want = want > p.ntiles ? p.ntiles : want;
    want = want > kD2MaxSplit ? kD2MaxSplit : want;
    p.per_split = (int)((p.ntiles + want - 1) / want);
    p.nsplit = (int)((p.ntiles + p.per_split - 1) / p.per_split);
    return true;
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_resnet_relu_gate_f32(const float* g, const float* y, float* out, long long total, mvsdet_stream_t stream) {
    MVS_REQUIRE(g && y && out, "resnet_relu_gate_f32: NULL pointer");
    MVS_REQUIRE(total >= 1 && blocks_of(total) < INT32_MAX, "resnet_relu_gate_f32: total=%lld must lie in 1 .. 2^31 blocks", total);
    MVS_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)y & 3u) == 0 && ((uintptr_t)out & 3u) == 0,
                "resnet_relu_gate_f32: the tensors must be 4-byte aligned");
    hipLaunchKernelGGL(resnet_relu_gate_kernel, dim3((unsigned)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, g, y, out, total);
    MVS_LAUNCH_CHECK("resnet_relu_gate_f32");
    return MVSDET_OK;
}

extern "C" int mvsdet_resnet_conv1x1_dx_bf16x3(const float* g, const void* wsplit, const float* residual, const float* gate, float* out, int N,
                                               int C, int Cout, int H, int W, int spread, mvsdet_stream_t stream) {
    MVS_REQUIRE(g && wsplit && out, "resnet_conv1x1_dx_bf16x3: NULL pointer");
    MVS_REQUIRE(N > 0 && H > 0 && W > 0, "resnet_conv1x1_dx_bf16x3: bad shape N=%d H=%d W=%d", N, H, W);
    MVS_REQUIRE(spread == 1 || spread == 2, "resnet_conv1x1_dx_bf16x3: the residual's stride=%d must be 1 or 2", spread);
    MVS_REQUIRE(Cout > 0 && Cout % kGemmBK == 0 && C > 0 && C % 32 == 0, "resnet_conv1x1_dx_bf16x3: Cout=%d must be a multiple of %d and C=%d of 32",
                Cout, kGemmBK, C);
    MVS_REQUIRE(C <= 65535 * kGemmBM, "resnet_conv1x1_dx_bf16x3: too many rows");
    MVS_REQUIRE((long long)H * W < INT32_MAX, "resnet_conv1x1_dx_bf16x3: map %d x %d too large", H, W);
    MVS_REQUIRE((long long)N * H * W <= INT32_MAX - kGemmBN, "resnet_conv1x1_dx_bf16x3: N H W = %lld columns exceed 2^31", (long long)N * H * W);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)g & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)residual & 3u) == 0 &&
                    ((uintptr_t)gate & 3u) == 0,
                "resnet_conv1x1_dx_bf16x3: wsplit must be 16-byte, the tensors 4-byte aligned");
    const int V = N * H * W, Hr = (H - 1) / 2 + 1, Wr = (W - 1) / 2 + 1;
    dim3 grid((unsigned)((V + kGemmBN - 1) / kGemmBN), (unsigned)((C + kGemmBM - 1) / kGemmBM));
    hipLaunchKernelGGL(resnet_dx1x1_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, g, static_cast<const uint4*>(wsplit), residual, gate, out,
                       C, Cout, H * W, W, V, spread, Hr * Wr, Wr);
    MVS_LAUNCH_CHECK("resnet_conv1x1_dx_bf16x3");
    return MVSDET_OK;
}

extern "C" int mvsdet_resnet_conv3x3_dx_bf16x3(const float* g, const void* wsplit, const float* gate, float* out, int N, int C, int Cout, int H,
                                               int W, int stride, mvsdet_stream_t stream) {
    MVS_REQUIRE(g && wsplit && out, "resnet_conv3x3_dx_bf16x3: NULL pointer");
    MVS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "resnet_conv3x3_dx_bf16x3: bad shape N=%d H=%d W=%d (1 <= N <= 65535)", N, H, W);
    MVS_REQUIRE(stride == 1 || stride == 2, "resnet_conv3x3_dx_bf16x3: stride=%d must be 1 or 2", stride);
    MVS_REQUIRE(Cout > 0 && Cout % kGemmBK == 0 && C > 0 && C % 32 == 0, "resnet_conv3x3_dx_bf16x3: Cout=%d must be a multiple of %d and C=%d of 32",
                Cout, kGemmBK, C);
    MVS_REQUIRE(C <= 65535 * kGemmBM && Cout <= INT32_MAX / 9, "resnet_conv3x3_dx_bf16x3: too many channels");
    MVS_REQUIRE((long long)H * W < INT32_MAX && (long long)N * H * W <= INT32_MAX - kGemmBN, "resnet_conv3x3_dx_bf16x3: map %d x %d of %d views too large",
                H, W, N);
    MVS_REQUIRE(((uintptr_t)wsplit & 15u) == 0 && ((uintptr_t)g & 3u) == 0 && ((uintptr_t)out & 3u) == 0 && ((uintptr_t)gate & 3u) == 0,
                "resnet_conv3x3_dx_bf16x3: wsplit must be 16-byte, the tensors 4-byte aligned");
    const unsigned row_blocks = (unsigned)((C + kGemmBM - 1) / kGemmBM);
    if (stride == 1) {
        using T = RnTile<1>;
        const long long tiles_x = (W + T::TW - 1) / T::TW, tiles_y = (H + T::TH - 1) / T::TH;
        MVS_GRANT_LDS("resnet_conv3x3_dx_bf16x3", resnet_dx3x3_s1_kernel, T::LdsBytes, T::LdsBytes);
        hipLaunchKernelGGL(resnet_dx3x3_s1_kernel, dim3((unsigned)(tiles_x * tiles_y), row_blocks, (unsigned)N), dim3(kThreads), T::LdsBytes,
                           (hipStream_t)stream, g, static_cast<const uint4*>(wsplit), gate, out, C, Cout, H, W, (int)tiles_x);
        MVS_LAUNCH_CHECK("resnet_conv3x3_dx_bf16x3");
        return MVSDET_OK;
    }
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const size_t mpad = (size_t)row_blocks * kGemmBM;
    size_t taps_before = 0;                                // the classes' matrices lie behind one another: (mpad, taps Cout) each
    for (int cls = 0; cls < 4; ++cls) {
        const int py = cls >> 1, px = cls & 1, Hc = (H - py + 1) / 2, Wc = (W - px + 1) / 2;
        const uint4* wc = static_cast<const uint4*>(wsplit) + mpad * taps_before * Cout / 4;   // 4 bytes a matrix element: hi and mid
        taps_before += (size_t)(1 + py) * (1 + px);
        if (Hc == 0 || Wc == 0) continue;                  // H = 1 or W = 1: no odd row or column
        const int V = N * Hc * Wc;
        hipLaunchKernelGGL(resnet_dx3x3_s2_kernel, dim3((unsigned)((V + kGemmBN - 1) / kGemmBN), row_blocks), dim3(kThreads), 0, (hipStream_t)stream,
                           g, wc, gate, out, C, Cout, H, W, Ho, Wo, py, px, Hc, Wc, V);
        MVS_LAUNCH_CHECK("resnet_conv3x3_dx_bf16x3 (stride 2)");
    }
    return MVSDET_OK;
}

extern "C" int mvsdet_resnet_dw_s2_splits(int taps, int N, int C, int Cout, int H, int W) {
    Dw2Plan p;
    return dw2_plan("resnet_dw_s2_splits", taps, N, C, Cout, H, W, p) ? p.nsplit : 0;
}

extern "C" size_t mvsdet_resnet_dw_s2_workspace_bytes(int taps, int N, int C, int Cout, int H, int W) {
    Dw2Plan p;
    if (!dw2_plan("resnet_dw_s2_workspace_bytes", taps, N, C, Cout, H, W, p)) return 0;
    return (size_t)p.nsplit * taps * Cout * C * sizeof(float);
}

extern "C" int mvsdet_resnet_dw_s2_bf16x3(const float* gy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int taps, int N,
                                          int C, int Cout, int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(gy && x && dw && workspace, "resnet_dw_s2_bf16x3: NULL pointer");
    Dw2Plan p;
    if (!dw2_plan("resnet_dw_s2_bf16x3", taps, N, C, Cout, H, W, p)) return MVSDET_ERR_INVALID_ARG;
    MVS_REQUIRE(((uintptr_t)gy & 3u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)dw & 3u) == 0 && ((uintptr_t)workspace & 3u) == 0,
                "resnet_dw_s2_bf16x3: the tensors and the workspace must be 4-byte aligned");
    MVS_REQUIRE_WORKSPACE("resnet_dw_s2_bf16x3", workspace_bytes, (size_t)p.nsplit * taps * Cout * C * sizeof(float));
    float* partial = static_cast<float*>(workspace);
    dim3 grid((unsigned)(C / kD2BC), (unsigned)(Cout / kD2BM), (unsigned)p.nsplit);
    if (taps == 9)
        hipLaunchKernelGGL(resnet_dw_s2_kernel<9>, grid, dim3(kThreads), 0, (hipStream_t)stream, gy, x, partial, C, Cout, H, W, p.Ho, p.Wo, p.tiles_x,
                           p.tiles_y, (int)p.ntiles, p.per_split);
    else
        hipLaunchKernelGGL(resnet_dw_s2_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, gy, x, partial, C, Cout, H, W, p.Ho, p.Wo, p.tiles_x,
                           p.tiles_y, (int)p.ntiles, p.per_split);
    MVS_LAUNCH_CHECK("resnet_dw_s2_bf16x3");
    const long long oc = (long long)Cout * C;
    hipLaunchKernelGGL(resnet_dw_s2_sum_kernel, dim3((unsigned)blocks_of(oc * taps)), dim3(kThreads), 0, (hipStream_t)stream, partial, dw, p.nsplit,
                       taps, oc);
    MVS_LAUNCH_CHECK("resnet_dw_s2_bf16x3 (sum)");
    return MVSDET_OK;
}
