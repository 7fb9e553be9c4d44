// The second reduction of stage 1: the group-wise correlation cost volume of the reference's lss_fpn.py:499-506,
//   corr[n,j,g,d,y,x] = (1/Cg) * sum over the Cg = C/G channels c of group g of  f[n,c,y,x] * warped_j[n,c,d,y,x],
// one (G,D,H,W) volume per neighbour j, fused with the warp: the K warped (C,D,H,W) volumes are never written.  warped_j is
// what homo_warp / homo_warp_pixel return for neighbour j: the positions come from sample_ray / sample_at / decode_sample /
// tap_weights of sweep_kernel.h and the tap sum is one product and three fused multiply-adds in the order nw, ne, sw, se, as in
// planesweep_pixel.hip, whose steps this file shares.  Zero padding, no z test, no mask; a NaN / inf position gives NaN.
//
// Depths are read through strides {view, hypothesis, pixel}: (N,D,H,W) per-pixel hypotheses, or (N,D) planes with pixel stride
// 0 -- the same kernel, no broadcast copy, and none of the plane form's footprint boxes or tables.
//
// Forward, plane_sweep_groupcorr_kernel<K, MODE>: block = (reference view, 128 consecutive pixels of the flattened map, unit),
// the lane map, decode, gathers and tap sums of the per-pixel form (pixel_form.h, shared with planesweep_pixel.hip).
// A channel group's sum is the lane's own channels of that group, then a butterfly over the slot's lanes on DPP (every lane
// ends with the same bits), then -- where a group spans several slabs -- the block's loop over those slabs, in registers:
//   MODE kCg4    Cg = 4    channel 8i + g is in the slab's group 2i + (g >> 2): one term per lane, butterfly over the quad;
//                          lane g stores group 2(g & 3) + (g >> 2)
//   MODE kCg8    Cg = 8    group i: one term per lane, butterfly over the 8 lanes; lanes g < 4 store group g
//   MODE kCg16   Cg = 16   group i >> 1: two terms per lane; lanes g < 2 store
//   MODE kCgSlabs Cg % 32 == 0   four terms per lane and slab, butterfly per slab, slabs summed in order; lane 0 of a slot stores
// No atomics: the same inputs give the same bits on every run.  With Cg in {4, 8, 16} C need not be a multiple of 32: the padded
// channels of the last slab belong to groups >= G, which are never stored.
//
// Units and XCDs.  A unit is what a block walks: ONE slab (Cg <= 16: it holds 32 / Cg whole groups) or the Cg / 32 consecutive
// slabs of ONE group.  Units are dealt as the pixel kernel deals slabs: unit u to XCD u mod 8, or, for fewer than 8 units that
// divide 8, an XCD owns a unit and one contiguous range of (view, tile) pairs.  An XCD's L2 then holds Cg / 32 slab images of a
// source view instead of one (614 KB each at 60x80); with one group over all of C = 256 that is every slab, 8 XCDs x one
// contiguous eighth of the (view, tile) pairs each -- the tiles of an XCD then share their neighbours' texels, which is what the
// dealing is for.  Splitting a group's slabs over blocks would need a second pass or atomics; the forward has neither.
//
// Stores: the lane's 4 pixels of one (neighbour, group, hypothesis) as one 16-byte non-temporal store where H*W % 4 == 0 (W % 4
// == 0 implies it: the map is walked flattened) and the output is 16-byte aligned, scalars otherwise.
//
// Backward, groupcorr_bwd_kernel<K>: dL/dfeat from g = dL/dcorr on the per-pixel form's backward steps (pixel_form.h: block =
// (view, 128 pixels, slab), one decode per (neighbour, pixel) into LDS, the recomputed warped value, the atomic scatter into the
// packed gradient map, the reference view's own term summed in LDS).  Its own: per hypothesis the block brings g / Cg of its
// slab's groups through LDS, and the coefficients are
//   reference view:  dL/df[c]        += sum_{j,d} g[j,grp(c),d] * warped_j[c] / Cg
//   neighbour j:     dL/dwarped_j[c]  = g[j,grp(c),d] * f[c] / Cg
// Atomic sums depend on arrival order: the last bits may differ from run to run.  Depths and proj get no gradient (module.py:115).
//
// Out of scope: fp16 storage, pitched output, view shards, the plane form's LDS footprint boxes for plane depths, other widths.
#include "pixel_form.h"

namespace mvsdet {
namespace {

enum { kCg4 = 0, kCg8 = 1, kCg16 = 2, kCgSlabs = 3 };

// v + the value of the lane CTRL names (a DPP control word): one butterfly step
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over the lane's quad (ALL = false) or over the 8 lanes of its pixel slot; every lane gets the same bits
template <bool ALL>
__device__ __forceinline__ float slot_sum(float v) {
    v = dpp_add<0xB1>(v);                      // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);                      // quad_perm:[2,3,0,1]
    if constexpr (ALL) v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the 8 lanes (its lanes all hold one value)
    return v;
}

template <int K, int MODE>
__global__ __launch_bounds__(kThreads) void plane_sweep_groupcorr_kernel(
    const float* __restrict__ packed, const int64_t* __restrict__ nbr, const float* __restrict__ proj, const float* __restrict__ depth,
    long long ds_n, long long ds_d, long long ds_p, float* __restrict__ corr, int N, int G, int S, int SG, int U, int D, int H, int W,
    int tiles, int d_per_block, int n_bt, int xcd_parts, float inv_cg, int vec) {
    constexpr int NR = MODE == kCgSlabs ? 1 : (MODE == kCg16 ? 2 : 4);   // group sums a lane carries per pixel
    constexpr int NGL = MODE == kCg4 ? 8 : (MODE == kCg8 ? 4 : (MODE == kCg16 ? 2 : 1));   // groups a unit puts out
    const int HW = H * W;
    int unit, bt;
    if (!pixel_block(blockIdx.x, U, n_bt, xcd_parts, unit, bt)) return;
    const int tile = bt % tiles, n = bt / tiles;
    const int d_begin = blockIdx.y * d_per_block, d_end = min(D, d_begin + d_per_block);
    const size_t slab_stride = (size_t)HW * kSlab;
    const int n_sl = MODE == kCgSlabs ? SG : 1;   // slabs the block walks
    const int slab0 = unit * n_sl;
    const float* ref_img = packed + ((size_t)n * S + slab0) * slab_stride;
    const char* nb_img[K];
#pragma unroll
    for (int j = 0; j < K; ++j) nb_img[j] = reinterpret_cast<const char*>(packed + (neighbour_view(nbr, n, K, j, N) * S + slab0) * slab_stride);
    const PixelLanes L = pixel_lanes(tile, HW);
    const int g = L.g, p0 = L.p0, st_n = L.st_n;

    // the lane's reference features (channels 8i + g of a slab) of its 4 pixels
    float f[4][4];
    auto load_ref = [&](int sl) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(ref_img + (size_t)sl * slab_stride + (size_t)min(p0 + s, HW - 1) * kSlab + 4 * g);
            f[s][0] = v.x; f[s][1] = v.y; f[s][2] = v.z; f[s][3] = v.w;
        }
    };
    load_ref(0);

    // the group this lane stores (after the butterfly every lane of the slot holds every sum) and which of its sums that is
    const int r_sel = MODE == kCg4 ? (g & 3) : (MODE == kCgSlabs ? 0 : g);
    const int lg = MODE == kCg4 ? 2 * (g & 3) + (g >> 2) : (MODE == kCgSlabs ? 0 : g);
    const int grp = unit * NGL + lg;
    const bool storer = (MODE == kCg4 || g < NGL) && grp < G && st_n > 0;

    const DecodeDuty<K> dd = decode_duty<K>(L, proj, n, H, W);
    const float* depth_px = depth + (size_t)n * ds_n + (size_t)dd.pdc * ds_p;   // hypothesis d of the decoded pixel: + d * ds_d
    float dv_next = d_begin < d_end ? depth_px[(size_t)d_begin * ds_d] : 0.0f;

    for (int d = d_begin; d < d_end; ++d) {
        const float dval = dv_next;
        if (d + 1 < d_end) dv_next = depth_px[(size_t)(d + 1) * ds_d];   // requested a hypothesis ahead
        int ro[K][4], rw[K][4];
        pixel_decode<K>(dd, dval, H, W, ro, rw);
        float out[K][4];   // [neighbour][pixel]: the sum this lane stores
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) out[j][s] = 0.0f;
        for (int sl = 0; sl < n_sl; ++sl) {
            if (n_sl > 1) load_ref(sl);   // block-uniform; a single slab's features were loaded once
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float4 tq[4][4];
                gather_4x4(nb_img[j] + (size_t)sl * slab_stride * sizeof(float), ro[j], L.g16, tq);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float w[4], r[NR];
                    step_weights(rw[j], s, w);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = warped_value(tq[s], w, i);
                        // the lane's own channels of a group: the first as a product, the others fused onto it
                        if constexpr (MODE == kCg4 || MODE == kCg8) r[i] = f[s][i] * v;
                        else if constexpr (MODE == kCg16) r[i >> 1] = (i & 1) ? fmaf(f[s][i], v, r[i >> 1]) : f[s][i] * v;
                        else r[0] = i ? fmaf(f[s][i], v, r[0]) : f[s][i] * v;
                    }
                    // over the slot's lanes; the lane keeps the sum it stores
                    float mine = 0.0f;
#pragma unroll
                    for (int k = 0; k < NR; ++k) {
                        const float t = slot_sum<MODE != kCg4>(r[k]);
                        mine = (k == r_sel) ? t : mine;
                    }
                    out[j][s] = out[j][s] + mine;   // slab after slab, in order (a single slab: 0 + sum, exact)
                }
            }
        }
        if (storer) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float* dst = corr + ((((size_t)n * K + j) * G + grp) * D + d) * HW + p0;
                if (vec && st_n == 4) {
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f vv = {out[j][0] * inv_cg, out[j][1] * inv_cg, out[j][2] * inv_cg, out[j][3] * inv_cg};
                    __builtin_nontemporal_store(vv, reinterpret_cast<v4f*>(dst));
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s < st_n) dst[s] = out[j][s] * inv_cg;
                }
            }
        }
    }
}

// lg_shift: a slab channel's group inside the slab is channel >> lg_shift (2, 3, 4; 5 where a group is one or more whole slabs);
// groups of slab s start at s * ngl (ngl = 32 / Cg) or are the one group s / SG.
template <int K>
__global__ __launch_bounds__(kThreads) void groupcorr_bwd_kernel(const float* __restrict__ packed, const int64_t* __restrict__ nbr,
                                                                  const float* __restrict__ proj, const float* __restrict__ depth,
                                                                  long long ds_n, long long ds_d, long long ds_p,
                                                                  const float* __restrict__ gcorr, float* __restrict__ gpacked, int N, int C,
                                                                  int G, int S, int SG, int ngl, int lg_shift, int D, int H, int W, int tiles,
                                                                  int d_per_block, float inv_cg) {
    constexpr int kPitch = kTilePix + 1;
    constexpr int kRows = 8;                       // at most 8 groups per slab (Cg = 4)
    __shared__ float s_g[K * kRows * kPitch];      // dL/dcorr / Cg of hypothesis d: [neighbour][group of the slab][pixel of the tile]
    __shared__ TapTables<K> s_tap;
    __shared__ float s_ref[kTilePix * kSlab];      // the reference view's own term, summed over the hypotheses
    const int HW = H * W;
    const PixelBwdBlock b = pixel_bwd_block(C, S, D, HW, tiles, d_per_block);   // c_ok: C = G * Cg, an existing channel is in an existing group
    const int n = b.n, tid = b.tid;
    const int lg = b.crow >> lg_shift;
    const int grp0 = ngl > 1 ? b.slab * ngl : b.slab / SG;        // first group of the slab
    const float* ref_img = packed + b.img + b.q;
    const float* nb_img[K];
    float* nb_grad[K];
    pixel_bwd_neighbours<K, false>(b, packed, gpacked, nbr, N, S, HW, nb_img, nb_grad);
    pixel_bwd_ref_zero(b, s_ref);
    for (int d = b.d_begin; d < b.d_end; ++d) {
        __syncthreads();   // every wave is done with the previous hypothesis' tables
        {   // dL/dcorr: thread = (pixel of the tile, every second row): 512 contiguous bytes per row
            const int pl = tid & (kTilePix - 1), pix = b.pix0 + pl;
            for (int r = tid >> 7; r < K * ngl; r += 2) {
                const int j = r / ngl, l = r - j * ngl, gg = grp0 + l;
                float v = 0.0f;
                if (pix < HW && gg < G) v = gcorr[((((size_t)n * K + j) * G + gg) * D + d) * HW + pix] * inv_cg;
                s_g[(j * kRows + l) * kPitch + pl] = v;
            }
        }
        pixel_bwd_decode<K>(b, proj, depth + (size_t)n * ds_n + (size_t)d * ds_d, (size_t)ds_p, H, W, s_tap);
        __syncthreads();
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int pl = pixel_bwd_pl(b, it), pix = b.pix0 + pl;
            if (pix >= HW) continue;
            const float fv = ref_img[(size_t)pix * kSlab];
            float coef[K];
            float own = 0.0f;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float go = s_g[(j * kRows + lg) * kPitch + pl];
                own = fmaf(go, tap_sum(nb_img[j], s_tap.off[j * kTilePix + pl], s_tap.w[j * kTilePix + pl]), own);
                coef[j] = go * fv;
            }
            s_ref[pl * kSlab + b.q] += own;
            if (b.c_ok) {
#pragma unroll
                for (int j = 0; j < K; ++j)
                    tap_scatter(nb_grad[j], s_tap.off[j * kTilePix + pl], s_tap.w[j * kTilePix + pl], s_tap.in[j * kTilePix + pl], coef[j]);
            }
        }
    }
    pixel_bwd_ref_flush(b, s_ref, gpacked, HW);
}

int gc_check(const char* name, const void* nbr, const void* proj, const float* depth, const int64_t* ds, int N, int K, int C, int G, int D,
             int H, int W) {
    MVS_REQUIRE(nbr && proj && depth && ds, "%s: NULL neighbour ids / proj / depth / depth_strides", name);
    if (int rc = pixel_shape_check(name, N, K, 1, C, D, H, W)) return rc;
    MVS_REQUIRE(gc_width_ok(C, G),
                "%s: C=%d G=%d: the group width C/G must divide C and be 4, 8, 16 or a multiple of 32 (C %% G == 0 and C/G in {4, 8, 16} "
                "or C/G %% 32 == 0)", name, C, G);
    MVS_REQUIRE(ds[0] >= 0 && ds[1] >= 0 && ds[2] >= 0, "%s: negative depth stride", name);
    MVS_REQUIRE(N <= 65535 && num_slabs(C) <= 65535, "%s: N or C too large (N and the slab count must be <= 65535)", name);
    return MVSDET_OK;
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_plane_sweep_groupcorr_packed_f32(const float* packed, const int64_t* nbr, const float* proj, const float* depth,
                                                       const int64_t* depth_strides, float* out, int N, int K, int C, int G, int D, int H,
                                                       int W, mvsdet_stream_t stream) {
    const char* name = "plane_sweep_groupcorr";
    MVS_REQUIRE(packed && out, "%s: NULL pointer", name);
    if (int rc = gc_check(name, nbr, proj, depth, depth_strides, N, K, C, G, D, H, W)) return rc;
    const int S = num_slabs(C), HW = H * W, cg = C / G;
    const int mode = cg == 4 ? kCg4 : (cg == 8 ? kCg8 : (cg == 16 ? kCg16 : kCgSlabs));
    const int SG = mode == kCgSlabs ? cg / kSlab : 1;
    const PixelBlocking pb = pixel_blocking(N, C, G, D, H, W, false);   // an XCD owns a unit
    const int U = pb.units;   // units: a group's slabs (mode kCgSlabs: G of them), or one slab of whole groups (S)
    const int tiles = pb.tiles, n_bt = pb.n_bt, dpb = pb.d_per_block;
    MVS_REQUIRE((D + dpb - 1) / dpb <= 65535, "%s: grid too large", name);
    const int vec = (HW % 4 == 0) && ((uintptr_t)out % 16 == 0);
    const float inv_cg = 1.0f / (float)cg;
    dim3 grid((unsigned)pb.grid_x, (unsigned)((D + dpb - 1) / dpb));
    hipStream_t st = (hipStream_t)stream;
    const long long ds_n = depth_strides[0], ds_d = depth_strides[1], ds_p = depth_strides[2];
#define MVS_GC_FWD(KV, MV)                                                                                                            \
    hipLaunchKernelGGL((plane_sweep_groupcorr_kernel<KV, MV>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, ds_n, ds_d, ds_p, \
                       out, N, G, S, SG, U, D, H, W, tiles, dpb, n_bt, pb.xcd_parts, inv_cg, vec)
#define MVS_GC_FWD_K(KV)                              \
    case KV:                                          \
        if (mode == kCg4) MVS_GC_FWD(KV, kCg4);       \
        else if (mode == kCg8) MVS_GC_FWD(KV, kCg8);  \
        else if (mode == kCg16) MVS_GC_FWD(KV, kCg16); \
        else MVS_GC_FWD(KV, kCgSlabs);                \
        break;
    switch (K) {
        MVS_GC_FWD_K(1)
        MVS_GC_FWD_K(2)
        MVS_GC_FWD_K(3)
        MVS_GC_FWD_K(4)
    }
#undef MVS_GC_FWD_K
#undef MVS_GC_FWD
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

extern "C" int mvsdet_plane_sweep_groupcorr_bwd_packed_f32(const float* packed, const int64_t* nbr, const float* proj, const float* depth,
                                                           const int64_t* depth_strides, const float* grad, float* gfeat, void* workspace,
                                                           size_t workspace_bytes, int N, int K, int C, int G, int D, int H, int W,
                                                           mvsdet_stream_t stream) {
    const char* name = "plane_sweep_groupcorr_bwd";
    MVS_REQUIRE(packed && grad && gfeat && workspace, "%s: NULL pointer", name);
    if (int rc = gc_check(name, nbr, proj, depth, depth_strides, N, K, C, G, D, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pixel_bwd_prologue(name, workspace, workspace_bytes, N, C, H, W, st)) return rc;
    float* gpacked = static_cast<float*>(workspace);
    const int S = num_slabs(C), cg = C / G;
    const int SG = cg >= kSlab ? cg / kSlab : 1, ngl = cg >= kSlab ? 1 : kSlab / cg;
    const int lg_shift = cg == 4 ? 2 : (cg == 8 ? 3 : (cg == 16 ? 4 : 5));
    const PixelBlocking pb = pixel_blocking(N, C, G, D, H, W, true);
    const int tiles = pb.tiles, dpb = pb.d_per_block;
    const float inv_cg = 1.0f / (float)cg;
    const long long ds_n = depth_strides[0], ds_d = depth_strides[1], ds_p = depth_strides[2];
    dim3 grid((unsigned)pb.grid_x, (unsigned)((D + dpb - 1) / dpb));
#define MVS_GC_BWD(KV)                                                                                                              \
    case KV:                                                                                                                        \
        hipLaunchKernelGGL((groupcorr_bwd_kernel<KV>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, ds_n, ds_d, ds_p, grad, \
                           gpacked, N, C, G, S, SG, ngl, lg_shift, D, H, W, tiles, dpb, inv_cg);                                    \
        break;
    switch (K) {
        MVS_GC_BWD(1)
        MVS_GC_BWD(2)
        MVS_GC_BWD(3)
        MVS_GC_BWD(4)
    }
#undef MVS_GC_BWD
    MVS_LAUNCH_CHECK(name);
    return pixel_unpack(gpacked, gfeat, N, C, H, W, st);
}
