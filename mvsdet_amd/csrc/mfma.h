// What every kernel on the bf16 matrix cores with three-term split operands ("bf16x3": costreg_bf16.hip's header has the arithmetic)
// shares: the fragment types, the 32x32 accumulator's row map, the fp32 -> (hi, mid) cut, the three-product step and the 128 x 64
// GEMM block over a pre-split weight matrix.  Included after common.h.
#pragma once

namespace mvsdet {

typedef short bf16x8 __attribute__((ext_vector_type(8)));     // an A or B fragment of v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16
typedef float f32x16 __attribute__((ext_vector_type(16)));    // a 32x32 accumulator
typedef float f32x4 __attribute__((ext_vector_type(4)));      // a 16x16 accumulator
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // a fragment as four bf16 pairs

// The 32x32 MFMA leaves column lane & 31 in a lane, and in register i of lane half `half` = lane >> 5 the row below: four consecutive
// rows per group of four registers, the two halves interleaved in steps of four, the groups eight rows apart.  New code writes
// `base + mfma32_row(i, half)`.  `first` is for costreg_conv0.hip and gshead.hip alone: it keeps the association (first + ...) their
// kernels were compiled and measured with, and goes with the next change that re-measures them.
__host__ __device__ constexpr int mfma32_row(int i, int half, int first = 0) { return first + (i & 3) + 8 * (i >> 2) + 4 * half; }

// fp32 -> the two bf16 pieces: hi = the value rounded to nearest even, mid = the remainder (exact in fp32) rounded once.  Two values at
// a time, as the packed conversion takes them; hi widens back to fp32 with a shift or a mask of the pair.
__device__ __forceinline__ unsigned bf16x3_pair(float a, float b) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const bf2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void bf16x3_split2(float f0, float f1, unsigned& hi, unsigned& mid) {
    hi = bf16x3_pair(f0, f1);
    mid = bf16x3_pair(f0 - __uint_as_float(hi << 16), f1 - __uint_as_float(hi & 0xffff0000u));
}
__device__ __forceinline__ void bf16x3_cut8(const float (&f)[8], u32x4& hi, u32x4& mid) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned h, m;
        bf16x3_split2(f[2 * p], f[2 * p + 1], h, m);
        hi[p] = h;
        mid[p] = m;
    }
}
__device__ __forceinline__ void bf16x3_cut8(const float (&f)[8], bf16x8& hi, bf16x8& mid) {
    u32x4 h, m;
    bf16x3_cut8(f, h, m);
    hi = __builtin_bit_cast(bf16x8, h);
    mid = __builtin_bit_cast(bf16x8, m);
}

// acc += A B with A = Ah + Am, B = Bh + Bm, without Am Bm (2^-16 of the product).  The two small products go first: they are added to
// each other and to the running sum before the large one, so their low bits are not rounded away against it one at a time.
__device__ __forceinline__ void bf16x3_mfma32(f32x16& acc, bf16x8 Ah, bf16x8 Am, bf16x8 Bh, bf16x8 Bm) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc, 0, 0, 0);
}
__device__ __forceinline__ void bf16x3_mfma16(f32x4& acc, bf16x8 Ah, bf16x8 Am, bf16x8 Bh, bf16x8 Bm) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Am, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, Bh, acc, 0, 0, 0);
}

// C[M][v] = A[M][K] B[K][v] with A a weight matrix cut ONCE per weight version by mvsdet_gemm_split_weight: M a multiple of kGemmBM,
// K of kGemmBK, laid out in fragment order [M/32][K/16][piece hi | mid][64 lanes][8 bf16], lane = 32 * (k-group of 8) + row of the
// tile, so that a wave's A fragment is 1 KiB of one coalesced load.  Every kernel that reads such a matrix takes its tile from here.
constexpr int kGemmBM = 128, kGemmBN = 64, kGemmBK = 32;

// One block's 128 rows x 64 columns: 4 waves, wave w = rows 32 w .. 32 w + 31 of the block x both 32-column tiles (acc[0], acc[1], which
// the caller has zeroed).  K in steps of 32: fetch(ks) leaves in f the 8 values k = 32 ks + 8 (tid >> 6) .. + 7 of column tid & 63 (zero
// past the last column); they are cut and written as two 16-byte units into the double-buffered stage s_b[stage][piece][k-group of 8]
// [column] (16 KiB), whose B fragments are conflict-free ds_read_b128.  The next step's values are fetched into registers before this
// step's MFMAs.  `f` MUST be the array that `fetch` fills (the caller's lambda captures it by reference): nothing checks it, and a
// fetch that fills another array multiplies stale values.  ws = the split matrix, m0 = the block's first row.  The stage is declared here and `fetch` taken by reference: as a
// parameter the stage costs 8 - 16 VGPRs (a wave per SIMD), `fetch` by value 118 instructions in fpn_lateral_kernel (docs/KERNEL_NOTES.md).
template <class Fetch>
__device__ __forceinline__ void gemm_bf16x3_block(f32x16 (&acc)[2], const float (&f)[8], const Fetch& fetch, const uint4* ws, int m0, int K,
                                                  int tid, int wave) {
    __shared__ uint4 s_b[2][2][4][kGemmBN];   // [stage][piece][k-group of 8][column]
    const int lane = tid & 63;
    auto put = [&](int buf) {
        u32x4 hi, mid;
        bf16x3_cut8(f, hi, mid);
        s_b[buf][0][tid >> 6][tid & 63] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        s_b[buf][1][tid >> 6][tid & 63] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    };
    const int rt = (m0 >> 5) + wave;                     // the wave's row tile
    const uint4* wa = ws + (size_t)rt * (K / 16) * 2 * 64 + lane;
    const int nks = K / kGemmBK;
    fetch(0);
    put(0);
    __syncthreads();
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nks) fetch(ks + 1);                 // in flight under the MFMAs below
        uint4 a_hi[2], a_mid[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            a_hi[s] = wa[((size_t)(2 * ks + s) * 2 + 0) * 64];
            a_mid[s] = wa[((size_t)(2 * ks + s) * 2 + 1) * 64];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 Ah = __builtin_bit_cast(bf16x8, a_hi[s]), Am = __builtin_bit_cast(bf16x8, a_mid[s]);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int kq = 2 * s + (lane >> 5), col = 32 * c + (lane & 31);
                bf16x3_mfma32(acc[c], Ah, Am, __builtin_bit_cast(bf16x8, s_b[buf][0][kq][col]), __builtin_bit_cast(bf16x8, s_b[buf][1][kq][col]));
            }
        }
        if (ks + 1 < nks) put(buf ^ 1);                  // the other stage: its readers finished before the last barrier
        __syncthreads();
    }
}

}  // namespace mvsdet
