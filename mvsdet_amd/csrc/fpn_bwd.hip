// Gradients of level 0 of the 2-D feature pyramid (fpn.hip has the forward and the module's definition):
//
//   g   = dL/dout0                                        (N,Cout,H0,W0), given
//   gL0 = conv3x3(g, w3'), w3'[c,o,dy,dx] = w3[o,c,2-dy,2-dx]     fpn_conv3x3_kernel on the flipped, transposed weight (no new kernel)
//   gL1 = up^T(gL0), gL2 = up^T(gL1), gL3 = up^T(gL2)     fpn_top_down_grad_kernel: adjoint of the nearest gather by size
//   dx_i = W_i^T gL_i                                     fpn_lateral_kernel on the split of W_i^T (no new kernel)
//   dW_i = sum over views and pixels of gL_i x_i^T        fpn_dw_kernel<1>;   db_i = sum of gL_i: fpn_bias_grad_kernel
//   dW3[o,c,dy,dx] = sum_{n,y,x} g[n,o,y,x] L0[n,c,y+dy-1,x+dx-1] (zero outside): fpn_dw_kernel<9>;   db3 = sum of g
//
// fpn_dw_kernel<TAPS>: a GEMM whose reduction index is the pixel, D[o][c] += A[o][k] B[k][c] per tap on v_mfma_f32_32x32x16_bf16, the 16 k
//   of one MFMA being 16 consecutive pixels of one row.  Both operands arrive as fp32 NCHW (pixel-contiguous, the order a fragment
//   wants), are cut into bf16 hi / mid with mfma.h's cut on the way into the LDS, and the three products mid hi, hi mid, hi hi are
//   accumulated in fp32, the small ones first.
//     block = 128 output channels x 32 input channels x all taps: wave w owns rows 32 w .. 32 w + 31 and TAPS accumulators (9 x 16
//             registers); the four waves share the X tile.
//     tile  = kDwTH x kDwTW = 2 x 16 pixels of gy and, for nine taps, the 4 x 18 halo of X; for one tap the 32 pixels are consecutive
//             pixels of one view (2 chunks of 16) and X has no halo.  An LDS row of X is 48 bytes as in costreg_dw_bf16.hip:
//             [x0 .. x0+7][x0+8 .. x0+15][(x0-2, x0-1) | (x0+16, x0+17) | pad]; the dx = 0 and dx = 2 fragments are formed from a lane's own
//             eight pixels, the other half's and the edge pairs with v_alignbit_b32.  Channel pitches of 5 and 13 (7) 16-byte units:
//             odd, so the ds_read_b128 of 16 lanes fall on 16 different bank quads.
//     stage = one LDS stage of 33 KiB, the next tile in registers under this tile's MFMAs (26 floats a thread), two barriers a tile;
//             two blocks per CU overlap each other's staging.  Padding and the ragged edge read a zero word: the ADDRESS is selected,
//             no load sits under a branch and nothing outside the two maps is read.
//     K     = the tiles (view-major) are dealt to `nsplit` blocks in contiguous runs; every split writes its fp32 partial
//             [split][tap][o][c] to the workspace and fpn_dw_sum_kernel adds the splits in ascending order into torch's (Cout,C,kh,kw).
//             No atomics: the same bits on every run.
//
// fpn_top_down_grad_kernel: one thread per element of the coarse map; its pre-image under the monotone index map is a range of rows
//   times a range of columns, summed rows ascending, then columns ascending.
// fpn_bias_grad_kernel: one block per channel, a thread's elements ascending, the block's sum on block_reduce.h.
#include "block_reduce.h"
#include "common.h"
#include "dw_sum.h"
#include "mfma.h"

namespace mvsdet {

constexpr int kDwTH = 2, kDwTW = 16;                  // the weight gradient's pixel tile (one tap: kDwTH chunks of kDwTW consecutive pixels)
constexpr int kDwBM = 128, kDwBC = 32;                // output x input channels of a block
constexpr int kDwSplitBlocks = 512;                   // K is split until about this many blocks run (two per CU)
constexpr int kDwGyChanB = kDwTH * 32 + 16;           // 80 B: 5 units
constexpr int kDwGyPieceB = kDwBM * kDwGyChanB;       // 10240
constexpr int kDwXRowB = 48;
constexpr int kDwMaxSplit = 65535;

template <int TAPS> struct DwShape {
    static constexpr int kXRows = TAPS == 9 ? kDwTH + 2 : kDwTH;
    static constexpr int kXChanB = kXRows * kDwXRowB + 16;     // 208 B = 13 units / 112 B = 7 units
    static constexpr int kXPieceB = kDwBC * kXChanB;
    static constexpr int kXUnits = kDwBC * kXRows * 2;          // (channel, row, half) units of 8 pixels: 256 / 128
    static constexpr int kXRounds = (kXUnits + kThreads - 1) / kThreads;
    static constexpr int kEdgeUnits = TAPS == 9 ? kDwBC * kXRows : 0;   // (channel, row) edge pairs: 128
    static_assert(kEdgeUnits <= kThreads, "one thread per edge pair");
};
constexpr int kDwGyPerRound = kThreads / (2 * kDwTH);         // 64 output channels of gy per staging round
constexpr int kDwGyRounds = kDwBM / kDwGyPerRound;            // 2

__device__ float4 g_fpn_zero;   // zero-initialised: the source of every padding element

// ATen's nearest source index (fpn.hip: fp_nearest)
__device__ __forceinline__ int fpb_nearest(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

// gy (N,Cout,H,W), x (N,C,H,W), partial [nsplit][TAPS][Cout][C]; grid (C/32, Cout/128, nsplit)
template <int TAPS>
__global__ __launch_bounds__(kThreads, 2) void fpn_dw_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                             float* __restrict__ partial, int C, int Cout, int H, int W, int tiles_x,
                                                             int tiles_y, int ntiles, int per_split) {
    using S = DwShape<TAPS>;
    __shared__ __attribute__((aligned(16))) char s_gy[2 * kDwGyPieceB];
    __shared__ __attribute__((aligned(16))) char s_x[2 * S::kXPieceB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = blockIdx.x * kDwBC, o0 = blockIdx.y * kDwBM, split = blockIdx.z;
    const size_t HW = (size_t)H * W;
    const float* const zero = reinterpret_cast<const float*>(&g_fpn_zero);

    // ---- staging roles, the same for every tile: gy unit (channel go + 64 a, row grow, half gh), X units, one edge pair
    const int gh = tid & 1, grow = (tid >> 1) & (kDwTH - 1), go = tid / (2 * kDwTH);
    const int g_lds = go * kDwGyChanB + grow * 32 + gh * 16;
    int xh[S::kXRounds], xrow[S::kXRounds], x_lds[S::kXRounds];
    const float* xchan[S::kXRounds];
#pragma unroll
    for (int a = 0; a < S::kXRounds; ++a) {
        const int u = min(tid + kThreads * a, S::kXUnits - 1), cr = u >> 1, xc = cr / S::kXRows;
        xh[a] = u & 1;
        xrow[a] = cr - xc * S::kXRows;
        x_lds[a] = xc * S::kXChanB + xrow[a] * kDwXRowB + xh[a] * 16;
        xchan[a] = x + (size_t)(c0 + xc) * HW;
    }
    const int el = min(tid, max(S::kEdgeUnits, 1) - 1), ec = el / S::kXRows, erow = el - ec * S::kXRows;
    const int e_lds = ec * S::kXChanB + erow * kDwXRowB + 32;
    const float* const echan = x + (size_t)(c0 + ec) * HW;
    const float* const gchan = gy + (size_t)(o0 + go) * HW;

    float fg[kDwGyRounds][8], fx[S::kXRounds][8], fe[2];
    // the tile (n, ty, tx): its values into registers.  One tap: tx = the tile of 32 consecutive pixels of the view, ty = 0.
    auto fetch = [&](int n, int ty, int tx) {
        const float* gv = gchan + (size_t)n * Cout * HW;
        const size_t xview = (size_t)n * C * HW;
        {
            long long off;
            int cnt;
            if (TAPS == 9) {
                const int y = ty * kDwTH + grow, xs = tx * kDwTW + 8 * gh;
                cnt = y < H ? W - xs : 0;
                off = (long long)y * W + xs;
            } else {
                off = (long long)tx * (kDwTH * kDwTW) + 16 * grow + 8 * gh;
                cnt = (int)min((long long)HW - off, (long long)8);
            }
#pragma unroll
            for (int a = 0; a < kDwGyRounds; ++a) {
                const float* p = gv + (size_t)(kDwGyPerRound * a) * HW + off;
#pragma unroll
                for (int j = 0; j < 8; ++j) fg[a][j] = *(j < cnt ? p + j : zero);
            }
        }
#pragma unroll
        for (int a = 0; a < S::kXRounds; ++a) {
            long long off;
            int cnt;
            if (TAPS == 9) {
                const int y = ty * kDwTH - 1 + xrow[a], xs = tx * kDwTW + 8 * xh[a];
                cnt = ((y >= 0) & (y < H)) ? W - xs : 0;
                off = (long long)y * W + xs;
            } else {
                off = (long long)tx * (kDwTH * kDwTW) + 16 * xrow[a] + 8 * xh[a];
                cnt = (int)min((long long)HW - off, (long long)8);
            }
            if (tid + kThreads * a >= S::kXUnits) cnt = 0;
            const float* p = xchan[a] + xview + off;
#pragma unroll
            for (int j = 0; j < 8; ++j) fx[a][j] = *(j < cnt ? p + j : zero);
        }
        if (TAPS == 9) {
            const int y = ty * kDwTH - 1 + erow, xl = tx * kDwTW - 1, xr = tx * kDwTW + kDwTW;
            const bool row_ok = (tid < S::kEdgeUnits) & (y >= 0) & (y < H);
            const float* p = echan + xview + (long long)y * W;
            fe[0] = *((row_ok & (xl >= 0)) ? p + xl : zero);
            fe[1] = *((row_ok & (xr < W)) ? p + xr : zero);
        }
    };
    // registers -> bf16 pieces in the LDS.  The values pass through an opaque statement first: without it the compiler cuts right
    // behind the loads, to save registers, and waits for them in front of the MFMAs they were to hide under.
    auto put = [&]() {
        u32x4 hi, mid;
#pragma unroll
        for (int a = 0; a < kDwGyRounds; ++a) {
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(fg[a][j]));
            bf16x3_cut8(fg[a], hi, mid);
            char* d = s_gy + g_lds + kDwGyPerRound * a * kDwGyChanB;
            *reinterpret_cast<uint4*>(d) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            *reinterpret_cast<uint4*>(d + kDwGyPieceB) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
        }
#pragma unroll
        for (int a = 0; a < S::kXRounds; ++a) {
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(fx[a][j]));
            bf16x3_cut8(fx[a], hi, mid);
            if (tid + kThreads * a < S::kXUnits) {
                char* d = s_x + x_lds[a];
                *reinterpret_cast<uint4*>(d) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                *reinterpret_cast<uint4*>(d + S::kXPieceB) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
            }
        }
        if (TAPS == 9) {
            asm volatile("" : "+v"(fe[0]));
            asm volatile("" : "+v"(fe[1]));
            unsigned h0, m0, h1, m1;
            bf16x3_split2(0.0f, fe[0], h0, m0);   // (x0-2: never read, x0-1)
            bf16x3_split2(fe[1], 0.0f, h1, m1);   // (x0+16, x0+17: never read)
            if (tid < S::kEdgeUnits) {
                char* d = s_x + e_lds;
                *reinterpret_cast<uint4*>(d) = make_uint4(h0, h1, 0u, 0u);
                *reinterpret_cast<uint4*>(d + S::kXPieceB) = make_uint4(m0, m1, 0u, 0u);
            }
        }
    };

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    const int r32 = lane & 31, hh = lane >> 5;
    const char* const ya = s_gy + (32 * wave + r32) * kDwGyChanB + hh * 16;
    const char* const xa = s_x + r32 * S::kXChanB;
    const int own_off = hh * 16, oth_off = 16 - hh * 16;

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
        for (int r = 0; r < kDwTH; ++r) {
            const bf16x8 Ah = *reinterpret_cast<const bf16x8*>(ya + r * 32);
            const bf16x8 Am = *reinterpret_cast<const bf16x8*>(ya + kDwGyPieceB + r * 32);
            if (TAPS == 9) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    // the mid pieces of X first (hi mid), then its hi pieces (mid hi, hi hi): per accumulator the two small products before
                    // the large one, and only one piece's fragments alive at a time; consecutive MFMAs go to different accumulators
#pragma unroll
                    for (int p = 1; p >= 0; --p) {
                        const char* rowp = xa + p * S::kXPieceB + (r + dy) * kDwXRowB;
                        const u32x4 own = *reinterpret_cast<const u32x4*>(rowp + own_off);   // this half's 8 pixels
                        u32x4 oth = *reinterpret_cast<const u32x4*>(rowp + oth_off);         // the other half's
                        u32x4 edg = *reinterpret_cast<const u32x4*>(rowp + 32);              // (x0-2, x0-1), (x0+16, x0+17)
                        // one word of each is used: keep the whole ds_read_b128, conflict-free at this channel pitch
                        asm volatile("" : "+v"(oth));
                        asm volatile("" : "+v"(edg));
                        const unsigned L = hh ? oth[3] : edg[0];     // high half = the pixel before own
                        const unsigned R = hh ? edg[1] : oth[0];     // low half = the pixel after own
                        const unsigned t1 = __builtin_amdgcn_alignbit(own[1], own[0], 16), t2 = __builtin_amdgcn_alignbit(own[2], own[1], 16),
                                       t3 = __builtin_amdgcn_alignbit(own[3], own[2], 16);
                        bf16x8 bq[3];
                        bq[0] = __builtin_bit_cast(bf16x8, (u32x4{__builtin_amdgcn_alignbit(own[0], L, 16), t1, t2, t3}));   // x-1
                        bq[1] = __builtin_bit_cast(bf16x8, own);                                                               // x
                        bq[2] = __builtin_bit_cast(bf16x8, (u32x4{t1, t2, t3, __builtin_amdgcn_alignbit(R, own[3], 16)}));   // x+1
                        if (p == 0) {
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) acc[(3 * dy + dx) % TAPS] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, bq[dx], acc[(3 * dy + dx) % TAPS], 0, 0, 0);
                        }
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) acc[(3 * dy + dx) % TAPS] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, bq[dx], acc[(3 * dy + dx) % TAPS], 0, 0, 0);
                    }
                }
            } else {
                const char* rowp = xa + r * kDwXRowB + own_off;
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

// dw (Cout,C,kh,kw)[o][c][tap] = the splits' partials added in ascending order (dw_sum.h); one thread per element
__global__ __launch_bounds__(kThreads) void fpn_dw_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw, int nsplit, int taps,
                                                              long long oc) {
    dw_sum_splits(partial, dw, nsplit, taps, oc);
}

// g (N,C,H,W) -> gt (N,C,Ht,Wt): gt[.., yt, xt] = sum of g over the pixels (y, x) whose nearest source is (yt, xt)
__global__ __launch_bounds__(kThreads) void fpn_top_down_grad_kernel(const float* __restrict__ g, float* __restrict__ gt, long long total,
                                                                     int H, int W, int Ht, int Wt, float scale_h, float scale_w) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const long long plane = e / ((long long)Ht * Wt);
    const int rem = (int)(e - plane * Ht * Wt), yt = rem / Wt, xt = rem - yt * Wt;
    // first destination index whose source is >= s: a guess from the scale, corrected on the map itself (it is monotone)
    auto first = [](int s, float scale, int in, int out) {
        int d = min(max((int)ceilf((float)s / scale), 0), out);
        while (d > 0 && fpb_nearest(d - 1, scale, in) >= s) --d;
        while (d < out && fpb_nearest(d, scale, in) < s) ++d;
        return d;
    };
    const int ya = first(yt, scale_h, Ht, H), yb = yt + 1 < Ht ? first(yt + 1, scale_h, Ht, H) : H;
    const int xa = first(xt, scale_w, Wt, W), xb = xt + 1 < Wt ? first(xt + 1, scale_w, Wt, W) : W;
    const float* gp = g + (size_t)plane * H * W;
    float s = 0.0f;
    for (int y = ya; y < yb; ++y)
        for (int xx = xa; xx < xb; ++xx) s = s + gp[(size_t)y * W + xx];
    gt[e] = s;
}

// db[c] = sum over views and pixels of g (N,C,H,W); block c
__global__ __launch_bounds__(kThreads) void fpn_bias_grad_kernel(const float* __restrict__ g, float* __restrict__ db, int N, int C, long long HW) {
    const int c = blockIdx.x;
    float a[1] = {0.0f};
    for (int n = 0; n < N; ++n) {
        const float* gp = g + ((size_t)n * C + c) * HW;
        for (long long p = threadIdx.x; p < HW; p += kThreads) a[0] = a[0] + gp[p];
    }
    if (block_sums(a)) db[c] = a[0];
}

struct DwPlan {
    int tiles_x, tiles_y, nsplit, per_split;
    long long ntiles;
};

// host only: the tiles and the split of K.  false: the shape is refused (the message is set)
static bool dw_plan(const char* who, int taps, int N, int C, int Cout, int H, int W, DwPlan& p) {
    if (taps != 1 && taps != 9) {
        set_error("%s: taps=%d must be 1 or 9", who, taps);
        return false;
    }
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0) {
        set_error("%s: bad shape N=%d H=%d W=%d (1 <= N <= 65535)", who, N, H, W);
        return false;
    }
    if (C <= 0 || C % kDwBC || Cout <= 0 || Cout % kDwBM || Cout / kDwBM > 65535) {
        set_error("%s: C=%d must be a multiple of %d and Cout=%d of %d", who, C, kDwBC, Cout, kDwBM);
        return false;
    }
    if ((long long)N * H * W >= INT32_MAX) {
        set_error("%s: N H W = %lld columns exceed 2^31", who, (long long)N * H * W);
        return false;
    }
    if (taps == 9) {
        p.tiles_x = (W + kDwTW - 1) / kDwTW;
        p.tiles_y = (H + kDwTH - 1) / kDwTH;
    } else {
        p.tiles_x = (int)(((long long)H * W + kDwTH * kDwTW - 1) / (kDwTH * kDwTW));
        p.tiles_y = 1;
    }
    p.ntiles = (long long)N * p.tiles_x * p.tiles_y;
    if (p.ntiles >= INT32_MAX) {
        set_error("%s: too many tiles", who);
        return false;
    }
    const long long per_k = (long long)(C / kDwBC) * (Cout / kDwBM);
    long long want = (kDwSplitBlocks + per_k - 1) / per_k;
    want = want < 1 ? 1 : want;
    want = want > p.ntiles ? p.ntiles : want;
    want = want > kDwMaxSplit ? kDwMaxSplit : want;
    p.per_split = (int)((p.ntiles + want - 1) / want);
    p.nsplit = (int)((p.ntiles + p.per_split - 1) / p.per_split);
    return true;
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_fpn_dw_splits(int taps, int N, int C, int Cout, int H, int W) {
    DwPlan p;
    return dw_plan("fpn_dw_splits", taps, N, C, Cout, H, W, p) ? p.nsplit : 0;
}

extern "C" size_t mvsdet_fpn_dw_workspace_bytes(int taps, int N, int C, int Cout, int H, int W) {
    DwPlan p;
    if (!dw_plan("fpn_dw_workspace_bytes", taps, N, C, Cout, H, W, p)) return 0;
    return (size_t)p.nsplit * taps * Cout * C * sizeof(float);
}

extern "C" int mvsdet_fpn_dw_bf16x3(const float* gy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int taps, int N, int C,
                                    int Cout, int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(gy && x && dw && workspace, "fpn_dw_bf16x3: NULL pointer");
    DwPlan p;
    if (!dw_plan("fpn_dw_bf16x3", taps, N, C, Cout, H, W, p)) return MVSDET_ERR_INVALID_ARG;
    MVS_REQUIRE(((uintptr_t)gy & 3u) == 0 && ((uintptr_t)x & 3u) == 0 && ((uintptr_t)dw & 3u) == 0 && ((uintptr_t)workspace & 3u) == 0,
                "fpn_dw_bf16x3: the tensors and the workspace must be 4-byte aligned");
    MVS_REQUIRE_WORKSPACE("fpn_dw_bf16x3", workspace_bytes, (size_t)p.nsplit * taps * Cout * C * sizeof(float));
    float* partial = static_cast<float*>(workspace);
    dim3 grid((unsigned)(C / kDwBC), (unsigned)(Cout / kDwBM), (unsigned)p.nsplit);
    if (taps == 9)
        hipLaunchKernelGGL(fpn_dw_kernel<9>, grid, dim3(kThreads), 0, (hipStream_t)stream, gy, x, partial, C, Cout, H, W, p.tiles_x, p.tiles_y,
                           (int)p.ntiles, p.per_split);
    else
        hipLaunchKernelGGL(fpn_dw_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, gy, x, partial, C, Cout, H, W, p.tiles_x, p.tiles_y,
                           (int)p.ntiles, p.per_split);
    MVS_LAUNCH_CHECK("fpn_dw_bf16x3");
    const long long oc = (long long)Cout * C;
    hipLaunchKernelGGL(fpn_dw_sum_kernel, dim3((unsigned)blocks_of(oc * taps)), dim3(kThreads), 0, (hipStream_t)stream, partial, dw, p.nsplit, taps,
                       oc);
    MVS_LAUNCH_CHECK("fpn_dw_bf16x3 (sum)");
    return MVSDET_OK;
}

extern "C" int mvsdet_fpn_top_down_grad_f32(const float* g, float* gt, int N, int C, int H, int W, int Ht, int Wt, mvsdet_stream_t stream) {
    MVS_REQUIRE(g && gt, "fpn_top_down_grad_f32: NULL pointer");
    MVS_REQUIRE(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "fpn_top_down_grad_f32: bad shape N=%d C=%d H=%d W=%d (1 <= N <= 65535)", N, C, H, W);
    MVS_REQUIRE(Ht >= 1 && Ht <= H && Wt >= 1 && Wt <= W, "fpn_top_down_grad_f32: the top level %d x %d must lie within 1 x 1 .. %d x %d", Ht, Wt, H,
                W);
    MVS_REQUIRE((long long)N * H * W < INT32_MAX && (long long)H * W < INT32_MAX, "fpn_top_down_grad_f32: N H W = %lld columns exceed 2^31",
                (long long)N * H * W);
    MVS_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)gt & 3u) == 0, "fpn_top_down_grad_f32: the tensors must be 4-byte aligned");
    const long long total = (long long)N * C * Ht * Wt;
    MVS_REQUIRE(blocks_of(total) < INT32_MAX, "fpn_top_down_grad_f32: too many elements");
    hipLaunchKernelGGL(fpn_top_down_grad_kernel, dim3((unsigned)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, g, gt, total, H, W, Ht, Wt,
                       (float)Ht / (float)H, (float)Wt / (float)W);
    MVS_LAUNCH_CHECK("fpn_top_down_grad_f32");
    return MVSDET_OK;
}

extern "C" int mvsdet_fpn_bias_grad_f32(const float* g, float* db, int N, int C, int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(g && db, "fpn_bias_grad_f32: NULL pointer");
    MVS_REQUIRE(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "fpn_bias_grad_f32: bad shape N=%d C=%d H=%d W=%d (1 <= N <= 65535)", N, C, H, W);
    MVS_REQUIRE((long long)N * H * W < INT32_MAX, "fpn_bias_grad_f32: N H W = %lld columns exceed 2^31", (long long)N * H * W);
    MVS_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)db & 3u) == 0, "fpn_bias_grad_f32: the tensors must be 4-byte aligned");
    hipLaunchKernelGGL(fpn_bias_grad_kernel, dim3((unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, g, db, N, C, (long long)H * W);
    MVS_LAUNCH_CHECK("fpn_bias_grad_f32");
    return MVSDET_OK;
}
