// The per-pixel form of the sweep, the steps its operators share: planesweep_pixel.hip (variance and compatibility warp at per-pixel
// depths) and groupcorr.hip (group-wise correlation) walk the same blocks with the same lanes and differ only in what they reduce
// the warped values to.  Each kernel's body is in its own file and calls the steps below; a change to the decode, the clamped
// taps, a tail pixel or the shape of the atomics is made here, once.
//
// The arithmetic is sweep_kernel.h's (sample_ray / sample_at / decode_sample / tap_weights) with the rounding points of
// oracle/planesweep_oracle.c mode 1: a tap sum is one product and three fused multiply-adds in the order nw, ne, sw, se.
//
// Forward: block = (reference view, 128 consecutive pixels of the flattened map, unit), a unit being a 32-channel slab or a run of
// slabs, dealt to the XCDs by pixel_block / pixel_grid.  Lanes are (pixel slot ps = lane >> 3, channel group g = lane & 7) and own
// 4 consecutive pixels x the 4 channels 8i + g of a slab, so
//   * a tap is ONE 16-byte load per lane straight from the packed maps, the 8 lanes of a slot covering the texel's 128 bytes;
//   * the decode duty is split over the 8 lanes of a slot: lane (ps, g) decodes the position of pixel-step g & 3 for neighbour
//     2p + (g >> 2) in pass p -- one position per lane, pass and hypothesis -- and the slot fetches offsets and weights with DPP.
//
// Backward: block = (view, 128 pixels, slab); per hypothesis the block decodes every (neighbour, pixel) once into LDS (TapTables);
// then lanes run over the 32 floats of a slab texel, two pixels per wave-instruction, recompute the warped values and scatter each
// tap gradient with atomicAdd(float*) into a packed gradient map in the workspace -- every atomic wave-instruction is two 128-byte
// texel segments (full rate on gfx950; one lane per row is an order of magnitude slower); only taps inside the source map add.  The
// reference view's own term is summed over the hypotheses in LDS and added once.  The packed gradient is then unpacked to (N,C,H,W)
// by pack.h's pass.  Atomic sums depend on arrival order: the gradient may differ in the last bits from run to run.
#pragma once
#include "common.h"

#include <algorithm>

#include "pack.h"
#include "sweep_kernel.h"

namespace mvsdet {

// quad_bcast / from_quad of sweep_kernel.h with the selector as a value (constant after unrolling)
__device__ __forceinline__ int quad_bcast_sel(int v, int s) {
    switch (s) {
        case 0: return quad_bcast<0>(v);
        case 1: return quad_bcast<1>(v);
        case 2: return quad_bcast<2>(v);
        default: return quad_bcast<3>(v);
    }
}
__device__ __forceinline__ int from_quad_sel(int v, int q) { return q == 0 ? from_quad<0>(v) : from_quad<1>(v); }

// byte offsets (texel * 128) of the four taps of a decoded position inside a slab image, clamped into the image: an outside
// tap reads an inside texel and carries weight * 0, as the plane kernel's gathered footprints do
__device__ __forceinline__ int4 tap_bytes(const SampleTaps& tp, int H, int W) {
    const int xa = clampi(tp.x0, 0, W - 1), xb = clampi(tp.x0 + 1, 0, W - 1);
    const int ya = clampi(tp.y0, 0, H - 1) * W, yb = clampi(tp.y0 + 1, 0, H - 1) * W;
    return make_int4((ya + xa) * 128, (ya + xb) * 128, (yb + xa) * 128, (yb + xb) * 128);
}

// block id -> (unit, view * tiles + tile): unit = id % U, or, for fewer than 8 units, an XCD owns a unit and takes one
// contiguous range of (view, tile) pairs (the plane kernel's dealing).  false: a padding block of the rounded-up grid.
__device__ __forceinline__ bool pixel_block(int id, int U, int n_bt, int xcd_parts, int& unit, int& bt) {
    unit = id % U;
    bt = id / U;
    if (xcd_parts > 1) {
        const int xcd = id & 7, k = id >> 3;
        const int per_part = (n_bt + xcd_parts - 1) / xcd_parts;
        unit = xcd % U;
        bt = (xcd / U) * per_part + k;
        if (k >= per_part) return false;
    }
    return bt < n_bt;
}

// neighbour j of view n, clamped into [0, N): never read outside the packed maps (ids are validated on the host)
__device__ __forceinline__ size_t neighbour_view(const int64_t* __restrict__ nbr, int n, int K, int j, int N) {
    const int64_t v = nbr[(size_t)n * K + j];
    return (size_t)(v < 0 ? 0 : (v >= N ? N - 1 : v));
}

// ---------------------------------------------------------------------------------------------------------------- forward
// The forward lane map of a tile.
struct PixelLanes {
    int g, g16;        // channel group of the lane; its 16 bytes of a texel
    int p0, st_n;      // the lane's 4 consecutive pixels of the flattened map; how many of them exist
};
__device__ __forceinline__ PixelLanes pixel_lanes(int tile, int HW) {
    PixelLanes L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ps = lane >> 3;
    L.g = lane & 7;
    L.g16 = L.g * 16;
    L.p0 = tile * kTilePix + 32 * wave + 4 * ps;
    L.st_n = max(0, min(4, HW - L.p0));
    return L;
}

// The lane's decode duty: the pixel p0 + (g & 3), neighbour 2p + (g >> 2) in pass p.  A struct of its own, filled after the
// kernel has requested its reference features: the projections' loads then issue together with those.  Filled with the lane map,
// the compiler waited for the projections before it requested the features -- a second round trip at the head of every block,
// and a block walks at most 4 hypotheses.
template <int K>
struct DecodeDuty {
    static constexpr int NP = (K + 1) / 2;   // decode passes: a lane decodes ONE (pixel-step, neighbour) pair per pass
    int pdc;           // the pixel this lane decodes, clamped into the map
    bool d_inside;     // ... and whether it exists
    SampleRay ray[NP > 0 ? NP : 1];
    float tr0[NP > 0 ? NP : 1], tr1[NP > 0 ? NP : 1], tr2[NP > 0 ? NP : 1];
};
template <int K>
__device__ __forceinline__ DecodeDuty<K> decode_duty(const PixelLanes& L, const float* __restrict__ proj, int n, int H, int W) {
    DecodeDuty<K> dd;
    const int HW = H * W;
    const int qd = L.g >> 2;
    const int pd = L.p0 + (L.g & 3);
    dd.d_inside = pd < HW;
    dd.pdc = min(pd, HW - 1);
    const int dy = dd.pdc / W, dx = dd.pdc - dy * W;
#pragma unroll
    for (int p = 0; p < DecodeDuty<K>::NP; ++p) {
        const float* P = proj + ((size_t)n * K + min(2 * p + qd, K - 1)) * 16;
        dd.ray[p] = sample_ray(P, (float)dx, (float)dy);
        dd.tr0[p] = P[3]; dd.tr1[p] = P[7]; dd.tr2[p] = P[11];
    }
    return dd;
}

// The decode passes of one hypothesis, dval being the depth of the lane's decoded pixel: per neighbour j the tap byte offsets
// ro[j][t] and weights rw[j][t] (float bits) of the slot's 4 pixel steps, one step per quad lane.
template <int K>
__device__ __forceinline__ void pixel_decode(const DecodeDuty<K>& dd, float dval, int H, int W, int (*ro)[4], int (*rw)[4]) {
#pragma unroll
    for (int p = 0; p < DecodeDuty<K>::NP; ++p) {
        // pixel outside the map: no tap inside, all weights +0 (nothing of it is stored)
        const float2 e_any = sample_at(dd.ray[p], dd.tr0[p], dd.tr1[p], dd.tr2[p], dval, H, W);
        const float2 e = dd.d_inside ? e_any : make_float2(kNoSample, kNoSample);
        const SampleTaps tp = decode_sample(e.x, e.y, H, W);
        const float4 dw = tap_weights(tp);
        const int4 dof = tap_bytes(tp, H, W);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * p + q;
            if (j < K) {
                ro[j][0] = from_quad_sel(dof.x, q); ro[j][1] = from_quad_sel(dof.y, q);
                ro[j][2] = from_quad_sel(dof.z, q); ro[j][3] = from_quad_sel(dof.w, q);
                rw[j][0] = from_quad_sel(__float_as_int(dw.x), q); rw[j][1] = from_quad_sel(__float_as_int(dw.y), q);
                rw[j][2] = from_quad_sel(__float_as_int(dw.z), q); rw[j][3] = from_quad_sel(__float_as_int(dw.w), q);
            }
        }
    }
}

// The lane's 4 pixels x 4 channels of one neighbour's slab image img, warped, in three steps: all 16 gathers of the neighbour are
// requested ahead of their arithmetic (tq[pixel step][tap]); the four weights of pixel step s; the tap sum of channel 8i + g of
// that step.  The tap sum is per value, not per step or neighbour, so that a kernel reduces each value where it arises: handing
// back 4 or 16 values at once made the compiler hold more gathers in flight and cost plane_sweep_groupcorr_kernel<1, kCgSlabs> and
// <4, kCg16> a wave per SIMD.
__device__ __forceinline__ void gather_4x4(const char* __restrict__ img, const int (&ro)[4], int g16, float4 (&tq)[4][4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) tq[s][t] = *reinterpret_cast<const float4*>(img + (quad_bcast_sel(ro[t], s) + g16));
}
__device__ __forceinline__ void step_weights(const int (&rw)[4], int s, float (&w)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) w[t] = __int_as_float(quad_bcast_sel(rw[t], s));
}
__device__ __forceinline__ float lane_of(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
__device__ __forceinline__ float warped_value(const float4 (&tq)[4], const float (&w)[4], int i) {
    float v = lane_of(tq[0], i) * w[0];
    v = fmaf(lane_of(tq[1], i), w[1], v);
    v = fmaf(lane_of(tq[2], i), w[2], v);
    v = fmaf(lane_of(tq[3], i), w[3], v);
    return v;
}

// --------------------------------------------------------------------------------------------------------------- backward
// What a backward block and its lanes work on.  Lanes run over the 32 floats of a slab texel, two pixels per wave-instruction.
struct PixelBwdBlock {
    int slab, n, pix0, d_begin, d_end;
    int tid, wave;
    int q, hw;      // float of the texel, which of the wave's two pixels
    int crow;       // packed float q = 4g + i <-> channel 8i + g of the slab
    bool c_ok;      // that channel exists
    size_t img;     // float offset of (view n, slab) inside the packed maps
};

__device__ __forceinline__ PixelBwdBlock pixel_bwd_block(int C, int S, int D, int HW, int tiles, int d_per_block) {
    PixelBwdBlock b;
    const int id = blockIdx.x, bt = id / S;
    b.slab = id % S;
    b.n = bt / tiles;
    b.pix0 = (bt % tiles) * kTilePix;
    b.d_begin = blockIdx.y * d_per_block;
    b.d_end = min(D, b.d_begin + d_per_block);
    b.tid = threadIdx.x;
    b.wave = b.tid >> 6;
    const int lane = b.tid & 63;
    b.q = lane & 31;
    b.hw = lane >> 5;
    b.crow = 8 * (b.q & 3) + (b.q >> 2);
    b.c_ok = b.slab * kSlab + b.crow < C;
    b.img = ((size_t)b.n * S + b.slab) * ((size_t)HW * kSlab);
    return b;
}

// pixel of the tile a lane works on in round it of 16
__device__ __forceinline__ int pixel_bwd_pl(const PixelBwdBlock& b, int it) { return 32 * b.wave + 2 * it + b.hw; }

// The lane's float of every neighbour's slab image (source; none where SELF) and of its gradient image.  SELF: the "neighbour"
// of batch row n is row n itself (the compatibility warp).
template <int K, bool SELF>
__device__ __forceinline__ void pixel_bwd_neighbours(const PixelBwdBlock& b, const float* __restrict__ packed, float* __restrict__ gpacked,
                                                     const int64_t* __restrict__ nbr, int N, int S, int HW, const float** nb_img,
                                                     float** nb_grad) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const size_t v = SELF ? (size_t)b.n : neighbour_view(nbr, b.n, K, j, N);
        const size_t at = (v * S + b.slab) * ((size_t)HW * kSlab) + b.q;
        nb_img[j] = SELF ? nullptr : packed + at;
        nb_grad[j] = gpacked + at;
    }
}

template <int KK>
struct TapTables {                    // one hypothesis of a tile, [neighbour][pixel of the tile]
    int4 off[KK * kTilePix];          // element offsets of the 4 taps inside a slab image (clamped into it)
    float4 w[KK * kTilePix];          // their weights (outside taps: weight * 0)
    unsigned in[KK * kTilePix];       // bit t: tap t lies inside the source map
};

// One decode per (neighbour, pixel) of the tile into LDS.  depth_d: the hypothesis' depth of the view's pixel 0, pixel stride ds_p.
template <int K, int KK>
__device__ __forceinline__ void pixel_bwd_decode(const PixelBwdBlock& b, const float* __restrict__ proj, const float* __restrict__ depth_d,
                                                 size_t ds_p, int H, int W, TapTables<KK>& s_tap) {
    const int HW = H * W;
    for (int task = b.tid; task < K * kTilePix; task += kThreads) {
        const int j = task >> 7, pl = task & (kTilePix - 1), pix = b.pix0 + pl;
        int4 off = make_int4(0, 0, 0, 0);
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned in = 0u;
        if (pix < HW) {
            const int y = pix / W, x = pix - y * W;
            const float* P = proj + ((size_t)b.n * K + j) * 16;
            const SampleRay r = sample_ray(P, (float)x, (float)y);
            const float2 e = sample_at(r, P[3], P[7], P[11], depth_d[(size_t)pix * ds_p], H, W);
            const SampleTaps tp = decode_sample(e.x, e.y, H, W);
            w = tap_weights(tp);
            const int4 bo = tap_bytes(tp, H, W);
            off = make_int4(bo.x >> 2, bo.y >> 2, bo.z >> 2, bo.w >> 2);
            in = (tp.x0in && tp.y0in ? 1u : 0u) | (tp.x1in && tp.y0in ? 2u : 0u) | (tp.x0in && tp.y1in ? 4u : 0u) |
                 (tp.x1in && tp.y1in ? 8u : 0u);
        }
        s_tap.off[task] = off;
        s_tap.w[task] = w;
        s_tap.in[task] = in;
    }
}

// the warped value recomputed from the tables: the lane's float of the four taps
__device__ __forceinline__ float tap_sum(const float* __restrict__ img, const int4& off, const float4& w) {
    float v = img[off.x] * w.x;
    v = fmaf(img[off.y], w.y, v);
    v = fmaf(img[off.z], w.z, v);
    v = fmaf(img[off.w], w.w, v);
    return v;
}

// dL/dwarped = coef through the four tap weights, the taps inside the source map only.  Two pixels x the 32 floats of a texel:
// every atomic wave-instruction is two 128-byte segments.
__device__ __forceinline__ void tap_scatter(float* __restrict__ grad, const int4& off, const float4& w, unsigned in, float coef) {
    if (in & 1u) atomicAdd(grad + off.x, coef * w.x);
    if (in & 2u) atomicAdd(grad + off.y, coef * w.y);
    if (in & 4u) atomicAdd(grad + off.z, coef * w.z);
    if (in & 8u) atomicAdd(grad + off.w, coef * w.w);
}

// s_ref [pixel of the tile][float of the texel]: the reference view's own term.  Every lane zeroes, sums into and flushes its
// own cells only.
__device__ __forceinline__ void pixel_bwd_ref_zero(const PixelBwdBlock& b, float* s_ref) {
#pragma unroll
    for (int it = 0; it < 16; ++it) s_ref[pixel_bwd_pl(b, it) * kSlab + b.q] = 0.0f;
}
__device__ __forceinline__ void pixel_bwd_ref_flush(const PixelBwdBlock& b, const float* s_ref, float* __restrict__ gpacked, int HW) {
    float* ref_grad = gpacked + b.img + b.q;
#pragma unroll 2
    for (int it = 0; it < 16; ++it) {
        const int pl = pixel_bwd_pl(b, it), pix = b.pix0 + pl;
        if (pix < HW && b.c_ok && b.d_begin < b.d_end) atomicAdd(ref_grad + (size_t)pix * kSlab, s_ref[pl * kSlab + b.q]);
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
// (static: pack.h's kernels are each translation unit's own)

// hypotheses per block: all of them unless the grid would be too small to fill the chip; option "pixel_dsplit" n > 0 sets the split
static int pixel_d_per_block(long long nblocks, int D, int at_most) {
    int dsplit = 1;
    if (options().pixel_dsplit > 0) dsplit = options().pixel_dsplit;
    else
        while (nblocks * dsplit < 2048 && dsplit < D) dsplit *= 2;
    dsplit = std::min(dsplit, D);
    int dpb = (D + dsplit - 1) / dsplit;
    if (at_most > 0) dpb = std::min(dpb, at_most);
    return dpb;
}

// what every entry of the per-pixel form asks of a shape; K in [k_min, MVSDET_MAX_NEIGHBORS]
static int pixel_shape_check(const char* name, int N, int K, int k_min, int C, int D, int H, int W) {
    MVS_REQUIRE(N > 0 && C > 0 && D > 0 && H > 1 && W > 1, "%s: bad shape N=%d C=%d D=%d H=%d W=%d", name, N, C, D, H, W);
    MVS_REQUIRE(K >= k_min && K <= MVSDET_MAX_NEIGHBORS, "%s: K=%d outside [%d,%d]", name, K, k_min, MVSDET_MAX_NEIGHBORS);
    MVS_REQUIRE(D <= MVSDET_MAX_DEPTH && H < 65535 && W < 65535, "%s: D > %d, or H or W > 65534", name, MVSDET_MAX_DEPTH);
    MVS_REQUIRE((size_t)H * W * kSlab * sizeof(float) < (size_t)INT32_MAX, "%s: one slab image exceeds 2^31 bytes", name);
    MVS_REQUIRE((size_t)D * H * W < (size_t)INT32_MAX, "%s: the depth hypotheses of one view exceed 2^31 elements", name);
    const long long tiles = ((long long)H * W + kTilePix - 1) / kTilePix;
    MVS_REQUIRE((long long)N * tiles * num_slabs(C) <= INT32_MAX / 2, "%s: grid too large", name);
    return MVSDET_OK;
}

// The forward grid over n_bt (view, tile) pairs x U units, for pixel_block: unit u to XCD u mod 8, or, for fewer than 8 units
// that divide 8, an XCD owns a unit and one contiguous range of pairs (compacted: the grid is rounded up).
struct PixelGrid {
    long long grid_x;
    int xcd_parts;
};
static PixelGrid pixel_grid(int n_bt, int U) {
    PixelGrid pg = {(long long)n_bt * U, 1};
    if (U < 8 && 8 % U == 0 && options().sweep_xcd != 0) {
        pg.xcd_parts = 8 / U;
        pg.grid_x = 8LL * ((n_bt + pg.xcd_parts - 1) / pg.xcd_parts);
    }
    return pg;
}

// the group widths the correlation is compiled for
static bool gc_width_ok(int C, int G) {
    if (G < 1 || C < 1 || C % G != 0) return false;
    const int cg = C / G;
    return cg == 4 || cg == 8 || cg == 16 || cg % 32 == 0;
}

// How a launch of the per-pixel form is cut into blocks: the ONE place every entry point and the query
// mvsdet_pixel_form_blocking take it from.  G = 0: variance / compatibility warp (a unit is a slab); G > 0: group correlation
// with G groups of a checked width (a unit is a slab of whole groups, or the slabs of one group).
//   forward:  grid (grid_x, ceil(D / d_per_block)), units dealt by pixel_block with xcd_parts; at most 4 hypotheses per block
//   backward: grid (N * tiles * S, ceil(D / d_per_block)), a unit is a slab (id % S), no XCD parts; no cap
struct PixelBlocking {
    int tiles, n_bt;    // 128-pixel tiles of a map; (view, tile) pairs
    int units, xcd_parts;
    long long grid_x;
    int d_per_block;
};
static PixelBlocking pixel_blocking(int N, int C, int G, int D, int H, int W, bool backward) {
    PixelBlocking pb;
    const int S = num_slabs(C);
    pb.tiles = (H * W + kTilePix - 1) / kTilePix;
    pb.n_bt = N * pb.tiles;
    if (backward) {
        pb.units = S;
        pb.xcd_parts = 1;
        pb.grid_x = (long long)pb.n_bt * S;
    } else {
        pb.units = (G > 0 && (C / G) % kSlab == 0) ? G : S;
        const PixelGrid pg = pixel_grid(pb.n_bt, pb.units);   // an XCD owns a unit
        pb.xcd_parts = pg.xcd_parts;
        pb.grid_x = pg.grid_x;
    }
    pb.d_per_block = pixel_d_per_block(pb.grid_x, D, backward ? 0 : 4);
    return pb;
}

// The backward's start: the workspace holds the packed gradient map, zeroed here for the atomics.
static int pixel_bwd_prologue(const char* name, void* workspace, size_t workspace_bytes, int N, int C, int H, int W, hipStream_t stream) {
    const size_t pb = mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W);
    MVS_REQUIRE_WORKSPACE(name, workspace_bytes, pb);
    MVS_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", name);
    MVS_REQUIRE(N <= 65535 && num_slabs(C) <= 65535, "%s: N or C too large", name);
    if (hipMemsetAsync(workspace, 0, pb, stream) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", name);
        return MVSDET_ERR_HIP;
    }
    return MVSDET_OK;
}

// ... and its end: the packed gradient map to (N,C,H,W)
static int pixel_unpack(const float* gpacked, float* gfeat, int N, int C, int H, int W, hipStream_t stream) {
    const int S = num_slabs(C), HW = H * W;
    if (HW % 4 == 0 && (uintptr_t)gfeat % 16 == 0) {
        dim3 dgrid((HW + 127) / 128, S, N);
        hipLaunchKernelGGL(unpack_features_dense_kernel, dgrid, dim3(kThreads), 0, stream, gpacked, gfeat, C, S, HW);
    } else {
        dim3 ugrid((HW + 63) / 64, S, N);
        hipLaunchKernelGGL(unpack_features_kernel, ugrid, dim3(kThreads), 0, stream, gpacked, gfeat, C, S, H, W);
    }
    MVS_LAUNCH_CHECK("unpack_features");
    return MVSDET_OK;
}

}  // namespace mvsdet
