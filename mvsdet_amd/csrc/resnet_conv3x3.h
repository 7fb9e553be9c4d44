// The main loop of the ResNet 3x3 convolution of stride 1 or 2 on a pre-split weight matrix (resnet.hip's header has the form): the tile,
// the halo staging and the nine taps' MFMAs.  The forward kernel (resnet.hip) and the stride-1 input gradient (resnet_bwd.hip: the same
// loop on the flipped, transposed weight) differ in their epilogues only.  Included after common.h and mfma.h.
#pragma once

namespace mvsdet {

// The 3x3 kernel's tile of stride S
template <int S>
struct RnTile {
    static constexpr int TW = 16, TH = S == 1 ? 8 : 4;         // output pixels of a block
    static constexpr int NT = TH / 2;                          // 32-pixel accumulators per wave: tile rows 2 t, 2 t + 1
    static constexpr int HW = S * (TW - 1) + 3, HH = S * (TH - 1) + 3;   // the halo: 18 x 10 | 33 x 9 input pixels
    static constexpr int Halo = HW * HH;
    static constexpr int Units = 4 * Halo;                     // (k-group of 8, halo pixel) staging units per 32 channels
    static constexpr int Rounds = (Units + kThreads - 1) / kThreads;
    static constexpr int Even = (HW + 1) / 2;                  // S = 2: even halo columns first, odd ones from here
    static constexpr size_t LdsBytes = (size_t)2 * 2 * 4 * Halo * sizeof(uint4);   // [stage][piece][k-group][halo pixel]
    // where halo column hx of a row is kept
    __host__ __device__ static constexpr int col(int hx) { return S == 1 ? hx : ((hx & 1) ? Even + (hx >> 1) : (hx >> 1)); }
};

// One block of conv3x3(x (N,Cin,H,W), stride S, zero padding 1) on ws = the split (ceil128(M), 9 Cin) tap-major matrix: view blockIdx.z,
// rows blockIdx.y * 128 + 32 wave .., output tile blockIdx.x.  Dynamic LDS: RnTile<S>::LdsBytes.  A wave whose rows lie below M ends in
// epilogue(acc, n, mw, y0, x0, lx, ly, half): accumulator t holds the output pixel (y0 + 2 t + ly, x0 + lx) (the caller masks the ragged
// edge), register i the row mw + mfma32_row(i, half).  A wave of padding rows stages and waits, no more.
template <int S, class Epilogue>
__device__ __forceinline__ void rn_conv3x3_block(const float* __restrict__ x, const uint4* __restrict__ ws, int M, int Cin, int H, int W,
                                                 int tiles_x, const Epilogue& epilogue) {
    using T = RnTile<S>;
    extern __shared__ uint4 s_rn[];                        // [stage][piece][k-group of 8][halo pixel]
    auto s_h = [&](int buf, int piece, int kq, int hp) -> uint4& { return s_rn[((buf * 2 + piece) * 4 + kq) * T::Halo + hp]; };
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, m0 = blockIdx.y * kGemmBM;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * T::TH, x0 = tx * T::TW;            // the tile's first output pixel
    const size_t HW = (size_t)H * W;

    // staging duties: unit u = tid + kThreads r -> k-group u / Halo, halo pixel u % Halo (zero outside the map)
    const float* xn = x + (size_t)n * Cin * HW;
    size_t soff[T::Rounds];
    bool sok[T::Rounds];
    int sdst[T::Rounds];
#pragma unroll
    for (int r = 0; r < T::Rounds; ++r) {
        const int u = tid + kThreads * r;
        const int kq = u / T::Halo, hp = u - kq * T::Halo;
        const int hy = hp / T::HW, hx = hp - hy * T::HW;
        const int y = S * y0 - 1 + hy, xx = S * x0 - 1 + hx;
        sdst[r] = kq * T::Halo + hy * T::HW + T::col(hx);
        sok[r] = u < T::Units && y >= 0 && y < H && xx >= 0 && xx < W;
        soff[r] = sok[r] ? (size_t)(8 * kq) * HW + (size_t)y * W + xx : 0;
    }
    float f[T::Rounds][8];
    auto fetch = [&](int chunk) {
        const float* xc = xn + (size_t)(chunk * kGemmBK) * HW;
#pragma unroll
        for (int r = 0; r < T::Rounds; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) f[r][j] = sok[r] ? xc[soff[r] + (size_t)j * HW] : 0.0f;
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int r = 0; r < T::Rounds; ++r) {
            if (tid + kThreads * r < T::Units) {
                u32x4 hi, mid;
                bf16x3_cut8(f[r], hi, mid);
                s_h(buf, 0, 0, sdst[r]) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                s_h(buf, 1, 0, sdst[r]) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
            }
        }
    };

    f32x16 acc[T::NT];
#pragma unroll
    for (int t = 0; t < T::NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    const int mw = m0 + 32 * wave;
    const bool live = mw < M;                              // wave-uniform: a wave of padding rows stages and waits, no more
    const int K16 = 9 * Cin / 16;
    const uint4* wa = ws + (size_t)(mw >> 5) * K16 * 2 * 64 + lane;
    // the lane's pixel inside accumulator t: tile row 2 t + ly, column lx; its halo pixel under tap (dy, dx) is row S (2 t + ly) + dy,
    // column S lx + dx
    const int lx = lane & 15, ly = (lane >> 4) & 1, half = lane >> 5;
    const int nch = Cin / kGemmBK;
    fetch(0);
    put(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) fetch(ch + 1);                   // in flight under the nine taps below
        if (live) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3, dx = tap - 3 * dy;
                const int k16 = (tap * Cin + ch * kGemmBK) / 16;
                // S = 2: column 2 lx + dx is the even lx (dx = 0), the odd lx (dx = 1) or the even lx + 1 (dx = 2)
                const int hcol = S == 1 ? lx + dx : (dx == 1 ? T::Even + lx : lx + (dx >> 1));
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 Ah = __builtin_bit_cast(bf16x8, wa[((size_t)(k16 + s) * 2 + 0) * 64]);
                    const bf16x8 Am = __builtin_bit_cast(bf16x8, wa[((size_t)(k16 + s) * 2 + 1) * 64]);
                    const int kq = 2 * s + half;
#pragma unroll
                    for (int t = 0; t < T::NT; ++t) {
                        const int hp = (S * (2 * t + ly) + dy) * T::HW + hcol;
                        const bf16x8 Bh = __builtin_bit_cast(bf16x8, s_h(buf, 0, kq, hp));
                        const bf16x8 Bm = __builtin_bit_cast(bf16x8, s_h(buf, 1, kq, hp));
                        bf16x3_mfma32(acc[t], Ah, Am, Bh, Bm);
                    }
                }
            }
        }
        if (ch + 1 < nch) put(buf ^ 1);                    // the other stage: its readers finished before the last barrier
        __syncthreads();
    }
    if (!live) return;
    epilogue(acc, n, mw, y0, x0, lx, ly, half);
}

}  // namespace mvsdet
