// Host half of the convolution entry points (costreg_bf16.hip, costreg_conv0.hip): what every one of them checks of its
// arguments, the fp32 view of an input tensor, the XCD-map predicate and the choice between the two tiles of the stride-2 and the
// transposed bf16x3 layers -- one copy each, so that a launcher and its size query, or two launchers, cannot drift apart.
// Host code only: nothing here is seen by a kernel.
#pragma once
#include "common.h"

// ---- the argument check: one refusal per macro, its wording here and nowhere else, the operator's name first ----
#define MVS_CONV_POINTERS(name, all_there) MVS_REQUIRE(all_there, "%s: NULL pointer", name)
#define MVS_CONV_AFFINE(name, scale, shift) MVS_REQUIRE(((scale) == nullptr) == ((shift) == nullptr), "%s: scale and shift come together", name)
#define MVS_CONV_SHAPE(name, N, Cin, D, H, W) \
    MVS_REQUIRE(N > 0 && Cin > 0 && D > 0 && H > 0 && W > 0, "%s: bad shape N=%d Cin=%d D=%d H=%d W=%d", name, N, Cin, D, H, W)
#define MVS_CONV_COUT(name, Cout) MVS_REQUIRE(Cout > 0 && Cout % 64 == 0, "%s: Cout=%d must be a multiple of 64", name, Cout)
// `addresses`: the weights and (scl) every SCL / PSCL buffer of the call, or-ed; a buffer that is not passed is 0
#define MVS_CONV_ALIGNED16(name, addresses, scl) \
    MVS_REQUIRE(((addresses) & 15u) == 0, "%s: %sweights must be 16-byte aligned", name, scl ? "SCL buffers and " : "")
// the transposed kernels write (and read the skip tensor as) float2: both w parities of an output pair
#define MVS_CONV_ALIGNED8(name, out, residual) \
    MVS_REQUIRE((((uintptr_t)(out) | (uintptr_t)(residual)) & 7u) == 0, "%s: out and residual must be 8-byte aligned", name)

namespace mvsdet {

// The check of the bf16x3 and fp16 + MX entry points, in their order.  (The fp32-MFMA pair of costreg_conv0.hip has checks of its
// own between these and Cout last: it lists the refusals itself, in its order, so that the one that wins stays the one that won.)
inline int conv_check_args(const char* name, bool pointers_there, const float* scale, const float* shift, int N, int Cin, int Cout,
                           int D, int H, int W, uintptr_t addresses16) {
    MVS_CONV_POINTERS(name, pointers_there);
    MVS_CONV_AFFINE(name, scale, shift);
    MVS_CONV_SHAPE(name, N, Cin, D, H, W);
    MVS_CONV_COUT(name, Cout);
    MVS_CONV_ALIGNED16(name, addresses16, true);
    return MVSDET_OK;
}

// ---- the fp32 view of an (N,C,D,H,W) input: element strides of n, c, d, h (w stride 1), the caller's or the contiguous ones ----
struct F32View { long long sN, sC, sD, sH; };
inline F32View f32_view(const int64_t* strides, int C, int D, int H, int W) {
    if (strides) return {strides[0], strides[1], strides[2], strides[3]};
    const unsigned long long vol = (unsigned long long)D * H * W;
    return {(long long)(C * vol), (long long)vol, (long long)H * W, (long long)W};
}
inline bool f32_view_ok(const F32View& v, int W) { return v.sN >= 0 && v.sC >= 0 && v.sD >= 0 && v.sH >= W; }
// `span31`: the kernel keeps a voxel's offset inside its channel volume in an int
inline int f32_view_check(const char* name, const F32View& v, int D, int H, int W, bool span31) {
    MVS_REQUIRE(f32_view_ok(v, W), "%s: bad strides", name);
    MVS_REQUIRE(!span31 || (long long)(D - 1) * v.sD + (long long)(H - 1) * v.sH + W < (1LL << 31),
                "%s: one channel volume spans more than 2^31 elements", name);
    return MVSDET_OK;
}

// Option "conv_xcd": an XCD takes a contiguous eighth of this grid (xcd_contiguous_id) -- where the eighths are whole and not tiny
inline int conv_xcd_map(const dim3& grid) {
    const long long blocks = (long long)grid.x * grid.y * grid.z;
    return options().conv_xcd != 0 && blocks % kXcds == 0 && blocks >= 64;
}

// ---- the tile of the stride-2 layer (over its OUTPUT extents) and of the transposed layer (over its INPUT extents):
// 4 x 8 x 16, or 3 x 16 x 8 where that pads (D, H, W) less; a tie goes to 4 x 8 x 16.  The number of input-channel splits
// follows from the 4 x 8 x 16 tiling whichever is taken (tiles416). ----
struct S2Tile {
    bool t38;
    int td, th, tw, tiles_d, tiles_h, tiles_w;
    long long tiles416, tiles;   // of the 4 x 8 x 16 tiling; of the tile taken
};
inline S2Tile s2_tile(int D, int H, int W) {
    const auto count = [&](int td, int th, int tw) { return (long long)((W + tw - 1) / tw) * ((H + th - 1) / th) * ((D + td - 1) / td); };
    S2Tile t;
    t.tiles416 = count(4, 8, 16);
    t.t38 = count(3, 16, 8) * (3 * 16 * 8) < t.tiles416 * (4 * 8 * 16);
    t.td = t.t38 ? 3 : 4; t.th = t.t38 ? 16 : 8; t.tw = t.t38 ? 8 : 16;
    t.tiles_d = (D + t.td - 1) / t.td; t.tiles_h = (H + t.th - 1) / t.th; t.tiles_w = (W + t.tw - 1) / t.tw;
    t.tiles = count(t.td, t.th, t.tw);
    return t;
}

}  // namespace mvsdet
