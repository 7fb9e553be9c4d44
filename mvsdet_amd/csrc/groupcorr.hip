// The second reduction of stage 1: the group-wise correlation cost volume of the reference's lss_fpn.py:499-506,
//   corr[n,j,g,d,y,x] = (1/Cg) * sum over the Cg = C/G channels c of group g of  f[n,c,y,x] * warped_j[n,c,d,y,x],
// one (G,D,H,W) volume per neighbour j, fused with the warp: the K warped (C,D,H,W) volumes are never written.  warped_j is
// what homo_warp / homo_warp_pixel return for neighbour j: the positions come from sample_ray / sample_at / decode_sample /
// tap_weights of sweep_kernel.h and the tap sum is one product and three fused multiply-adds in the order nw, ne, sw, se, as in
// planesweep_pixel.hip, the model of this file.  Zero padding, no z test, no mask; a NaN / inf position gives NaN.
//
// Depths are read through strides {view, hypothesis, pixel}: (N,D,H,W) per-pixel hypotheses, or (N,D) planes with pixel stride
// 0 -- the same kernel, no broadcast copy, and none of the plane form's footprint boxes or tables.
//
// Forward, plane_sweep_groupcorr_kernel<K, MODE>: block = (reference view, 128 consecutive pixels of the flattened map, unit),
// lanes (pixel slot ps = lane >> 3, channel group of lanes g = lane & 7) owning 4 consecutive pixels x the 4 channels 8i + g of
// a slab, a tap = one 16-byte gather per lane, the decode duty split over the 8 lanes of a slot: all as in the pixel kernel.
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
// Backward, groupcorr_bwd_kernel<K>: dL/dfeat from g = dL/dcorr, the structure of sweep_pixel_bwd_kernel: block = (view, 128
// pixels, slab); per hypothesis the block brings g / Cg of its slab's groups through LDS, decodes every (neighbour, pixel) once
// into LDS, and lanes run over the 32 floats of a slab texel, two pixels per wave-instruction, recomputing the warped values:
//   reference view:  dL/df[c]        += sum_{j,d} g[j,grp(c),d] * warped_j[c] / Cg   summed over the hypotheses in LDS, added once
//   neighbour j:     dL/dwarped_j[c]  = g[j,grp(c),d] * f[c] / Cg                    scattered through the four tap weights with
// atomicAdd(float*) into the packed gradient map of the workspace (two 128-byte texel segments per wave-instruction; only taps
// inside the source map add), unpacked by pack.h's pass.  Atomic sums depend on arrival order: the last bits may differ from run
// to run.  Depths and proj get no gradient (module.py:115).
//
// Out of scope: fp16 storage, pitched output, view shards, the plane form's LDS footprint boxes for plane depths, other widths.
#include "common.h"

#include <algorithm>

#include "pack.h"
#include "sweep_kernel.h"

namespace mvsdet {
namespace {

enum { kCg4 = 0, kCg8 = 1, kCg16 = 2, kCgSlabs = 3 };

// the pixel kernel's small helpers (planesweep_pixel.hip keeps them to itself): DPP selectors as values, tap byte offsets
// clamped into the image (an outside tap reads an inside texel and carries weight * 0), block id -> (unit, view * tiles + tile)
__device__ __forceinline__ int gc_quad_bcast(int v, int s) {
    switch (s) {
        case 0: return quad_bcast<0>(v);
        case 1: return quad_bcast<1>(v);
        case 2: return quad_bcast<2>(v);
        default: return quad_bcast<3>(v);
    }
}
__device__ __forceinline__ int gc_from_quad(int v, int q) { return q == 0 ? from_quad<0>(v) : from_quad<1>(v); }
__device__ __forceinline__ int4 gc_tap_bytes(const SampleTaps& tp, int H, int W) {
    const int xa = clampi(tp.x0, 0, W - 1), xb = clampi(tp.x0 + 1, 0, W - 1);
    const int ya = clampi(tp.y0, 0, H - 1) * W, yb = clampi(tp.y0 + 1, 0, H - 1) * W;
    return make_int4((ya + xa) * 128, (ya + xb) * 128, (yb + xa) * 128, (yb + xb) * 128);
}
__device__ __forceinline__ bool gc_block(int id, int U, int n_bt, int xcd_parts, int& unit, int& bt) {
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
    constexpr int NP = (K + 1) / 2;   // decode passes: a lane decodes ONE (pixel-step, neighbour) pair per pass
    constexpr int NR = MODE == kCgSlabs ? 1 : (MODE == kCg16 ? 2 : 4);   // group sums a lane carries per pixel
    constexpr int NGL = MODE == kCg4 ? 8 : (MODE == kCg8 ? 4 : (MODE == kCg16 ? 2 : 1));   // groups a unit puts out
    const int HW = H * W;
    int unit, bt;
    if (!gc_block(blockIdx.x, U, n_bt, xcd_parts, unit, bt)) return;
    const int tile = bt % tiles, n = bt / tiles;
    const int d_begin = blockIdx.y * d_per_block, d_end = min(D, d_begin + d_per_block);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane & 7, ps = lane >> 3;
    const size_t slab_stride = (size_t)HW * kSlab;
    const int n_sl = MODE == kCgSlabs ? SG : 1;   // slabs the block walks
    const int slab0 = unit * n_sl;
    const float* ref_img = packed + ((size_t)n * S + slab0) * slab_stride;
    const char* nb_img[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int64_t v = nbr[(size_t)n * K + j];
        v = v < 0 ? 0 : (v >= N ? N - 1 : v);   // never read outside the packed maps (ids are validated on the host)
        nb_img[j] = reinterpret_cast<const char*>(packed + ((size_t)v * S + slab0) * slab_stride);
    }
    const int g16 = g * 16;   // the lane's 16 bytes of a texel

    // the lane's 4 consecutive pixels of the flattened map and their reference features (channels 8i + g of a slab)
    const int p0 = tile * kTilePix + 32 * wave + 4 * ps;
    const int st_n = max(0, min(4, HW - p0));   // how many of the 4 pixels exist
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

    // decode duty: the pixel p0 + (g & 3), neighbour 2p + (g >> 2) in pass p
    const int qd = g >> 2;
    const int pd = p0 + (g & 3);
    const bool d_inside = pd < HW;
    const int pdc = min(pd, HW - 1);
    const int dy = pdc / W, dx = pdc - dy * W;
    SampleRay ray[NP];
    float tr0[NP], tr1[NP], tr2[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float* P = proj + ((size_t)n * K + min(2 * p + qd, K - 1)) * 16;
        ray[p] = sample_ray(P, (float)dx, (float)dy);
        tr0[p] = P[3]; tr1[p] = P[7]; tr2[p] = P[11];
    }
    const float* depth_px = depth + (size_t)n * ds_n + (size_t)pdc * ds_p;   // hypothesis d of the decoded pixel: + d * ds_d
    float dv_next = d_begin < d_end ? depth_px[(size_t)d_begin * ds_d] : 0.0f;

    for (int d = d_begin; d < d_end; ++d) {
        const float dval = dv_next;
        if (d + 1 < d_end) dv_next = depth_px[(size_t)(d + 1) * ds_d];   // requested a hypothesis ahead
        int ro[K][4], rw[K][4];   // per neighbour: the tap offsets and weights of the slot's 4 pixel steps, one per quad lane
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            // pixel outside the map: no tap inside, all weights +0 (nothing of it is stored)
            const float2 e_any = sample_at(ray[p], tr0[p], tr1[p], tr2[p], dval, H, W);
            const float2 e = d_inside ? e_any : make_float2(kNoSample, kNoSample);
            const SampleTaps tp = decode_sample(e.x, e.y, H, W);
            const float4 dw = tap_weights(tp);
            const int4 dof = gc_tap_bytes(tp, H, W);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = 2 * p + q;
                if (j < K) {
                    ro[j][0] = gc_from_quad(dof.x, q); ro[j][1] = gc_from_quad(dof.y, q);
                    ro[j][2] = gc_from_quad(dof.z, q); ro[j][3] = gc_from_quad(dof.w, q);
                    rw[j][0] = gc_from_quad(__float_as_int(dw.x), q); rw[j][1] = gc_from_quad(__float_as_int(dw.y), q);
                    rw[j][2] = gc_from_quad(__float_as_int(dw.z), q); rw[j][3] = gc_from_quad(__float_as_int(dw.w), q);
                }
            }
        }
        float out[K][4];   // [neighbour][pixel]: the sum this lane stores
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) out[j][s] = 0.0f;
        for (int sl = 0; sl < n_sl; ++sl) {
            if (n_sl > 1) load_ref(sl);   // block-uniform; a single slab's features were loaded once
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const char* img = nb_img[j] + (size_t)sl * slab_stride * sizeof(float);
                float4 tq[4][4];
#pragma unroll
                for (int s = 0; s < 4; ++s)   // all 16 gathers of a neighbour requested ahead of their arithmetic
#pragma unroll
                    for (int t = 0; t < 4; ++t) tq[s][t] = *reinterpret_cast<const float4*>(img + (gc_quad_bcast(ro[j][t], s) + g16));
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float w0 = __int_as_float(gc_quad_bcast(rw[j][0], s)), w1 = __int_as_float(gc_quad_bcast(rw[j][1], s));
                    const float w2 = __int_as_float(gc_quad_bcast(rw[j][2], s)), w3 = __int_as_float(gc_quad_bcast(rw[j][3], s));
                    const float t0[4] = {tq[s][0].x, tq[s][0].y, tq[s][0].z, tq[s][0].w};
                    const float t1[4] = {tq[s][1].x, tq[s][1].y, tq[s][1].z, tq[s][1].w};
                    const float t2[4] = {tq[s][2].x, tq[s][2].y, tq[s][2].z, tq[s][2].w};
                    const float t3[4] = {tq[s][3].x, tq[s][3].y, tq[s][3].z, tq[s][3].w};
                    float r[NR];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = t0[i] * w0;
                        v = fmaf(t1[i], w1, v);
                        v = fmaf(t2[i], w2, v);
                        v = fmaf(t3[i], w3, v);
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
    __shared__ int4 s_off[K * kTilePix];           // element offsets of the 4 taps inside a slab image (clamped into it)
    __shared__ float4 s_w[K * kTilePix];           // their weights (outside taps: weight * 0)
    __shared__ unsigned s_in[K * kTilePix];        // bit t: tap t lies inside the source map
    __shared__ float s_ref[kTilePix * kSlab];      // the reference view's own term, summed over the hypotheses
    const int HW = H * W;
    const int id = blockIdx.x;
    const int slab = id % S, bt = id / S;
    const int tile = bt % tiles, n = bt / tiles;
    const int pix0 = tile * kTilePix;
    const int d_begin = blockIdx.y * d_per_block, d_end = min(D, d_begin + d_per_block);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slab_stride = (size_t)HW * kSlab;
    const int q = lane & 31, hw = lane >> 5;                      // float of the texel, which of the wave's two pixels
    const int crow = 8 * (q & 3) + (q >> 2);                      // packed float q = 4g + i <-> channel 8i + g of the slab
    const bool c_ok = slab * kSlab + crow < C;                    // C = G * Cg: an existing channel is in an existing group
    const int lg = crow >> lg_shift;
    const int grp0 = ngl > 1 ? slab * ngl : slab / SG;            // first group of the slab
    const float* ref_img = packed + ((size_t)n * S + slab) * slab_stride + q;
    const float* nb_img[K];
    float* nb_grad[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int64_t v = nbr[(size_t)n * K + j];
        v = v < 0 ? 0 : (v >= N ? N - 1 : v);
        nb_img[j] = packed + ((size_t)v * S + slab) * slab_stride + q;
        nb_grad[j] = gpacked + ((size_t)v * S + slab) * slab_stride + q;
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) s_ref[(32 * wave + 2 * it + hw) * kSlab + q] = 0.0f;   // the lane's own cells throughout
    for (int d = d_begin; d < d_end; ++d) {
        __syncthreads();   // every wave is done with the previous hypothesis' tables
        {   // dL/dcorr: thread = (pixel of the tile, every second row): 512 contiguous bytes per row
            const int pl = tid & (kTilePix - 1), pix = pix0 + pl;
            for (int r = tid >> 7; r < K * ngl; r += 2) {
                const int j = r / ngl, l = r - j * ngl, gg = grp0 + l;
                float v = 0.0f;
                if (pix < HW && gg < G) v = gcorr[((((size_t)n * K + j) * G + gg) * D + d) * HW + pix] * inv_cg;
                s_g[(j * kRows + l) * kPitch + pl] = v;
            }
        }
        for (int task = tid; task < K * kTilePix; task += kThreads) {   // one decode per (neighbour, pixel)
            const int j = task >> 7, pl = task & (kTilePix - 1), pix = pix0 + pl;
            int4 off = make_int4(0, 0, 0, 0);
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            unsigned in = 0u;
            if (pix < HW) {
                const int y = pix / W, x = pix - y * W;
                const float* P = proj + ((size_t)n * K + j) * 16;
                const SampleRay r = sample_ray(P, (float)x, (float)y);
                const float dval = depth[(size_t)n * ds_n + (size_t)d * ds_d + (size_t)pix * ds_p];
                const float2 e = sample_at(r, P[3], P[7], P[11], dval, H, W);
                const SampleTaps tp = decode_sample(e.x, e.y, H, W);
                w = tap_weights(tp);
                const int4 b = gc_tap_bytes(tp, H, W);
                off = make_int4(b.x >> 2, b.y >> 2, b.z >> 2, b.w >> 2);
                in = (tp.x0in && tp.y0in ? 1u : 0u) | (tp.x1in && tp.y0in ? 2u : 0u) | (tp.x0in && tp.y1in ? 4u : 0u) |
                     (tp.x1in && tp.y1in ? 8u : 0u);
            }
            s_off[task] = off;
            s_w[task] = w;
            s_in[task] = in;
        }
        __syncthreads();
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int pl = 32 * wave + 2 * it + hw, pix = pix0 + pl;
            if (pix >= HW) continue;
            const float fv = ref_img[(size_t)pix * kSlab];
            float coef[K];
            float own = 0.0f;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float go = s_g[(j * kRows + lg) * kPitch + pl];
                const int4 off = s_off[j * kTilePix + pl];
                const float4 w = s_w[j * kTilePix + pl];
                float v = nb_img[j][off.x] * w.x;
                v = fmaf(nb_img[j][off.y], w.y, v);
                v = fmaf(nb_img[j][off.z], w.z, v);
                v = fmaf(nb_img[j][off.w], w.w, v);
                own = fmaf(go, v, own);
                coef[j] = go * fv;
            }
            s_ref[pl * kSlab + q] += own;
            if (c_ok) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int4 off = s_off[j * kTilePix + pl];
                    const float4 w = s_w[j * kTilePix + pl];
                    const unsigned in = s_in[j * kTilePix + pl];
                    // two pixels x the 32 floats of a texel: every atomic wave-instruction is two 128-byte segments
                    if (in & 1u) atomicAdd(nb_grad[j] + off.x, coef[j] * w.x);
                    if (in & 2u) atomicAdd(nb_grad[j] + off.y, coef[j] * w.y);
                    if (in & 4u) atomicAdd(nb_grad[j] + off.z, coef[j] * w.z);
                    if (in & 8u) atomicAdd(nb_grad[j] + off.w, coef[j] * w.w);
                }
            }
        }
    }
    float* ref_grad = gpacked + ((size_t)n * S + slab) * slab_stride + q;
#pragma unroll 2
    for (int it = 0; it < 16; ++it) {
        const int pl = 32 * wave + 2 * it + hw, pix = pix0 + pl;
        if (pix < HW && c_ok && d_begin < d_end) atomicAdd(ref_grad + (size_t)pix * kSlab, s_ref[pl * kSlab + q]);
    }
}

// hypotheses per block: all of them unless the grid would be too small to fill the chip
int gc_d_per_block(long long nblocks, int D, int at_most) {
    int dsplit = 1;
    while (nblocks * dsplit < 2048 && dsplit < D) dsplit *= 2;
    dsplit = std::min(dsplit, D);
    int dpb = (D + dsplit - 1) / dsplit;
    if (at_most > 0) dpb = std::min(dpb, at_most);
    return dpb;
}

bool gc_width_ok(int C, int G) {
    if (G < 1 || C < 1 || C % G != 0) return false;
    const int cg = C / G;
    return cg == 4 || cg == 8 || cg == 16 || cg % 32 == 0;
}

int gc_check(const char* name, const void* nbr, const void* proj, const float* depth, const int64_t* ds, int N, int K, int C, int G, int D,
             int H, int W) {
    MVS_REQUIRE(nbr && proj && depth && ds, "%s: NULL neighbour ids / proj / depth / depth_strides", name);
    MVS_REQUIRE(N > 0 && C > 0 && D > 0 && H > 1 && W > 1, "%s: bad shape N=%d C=%d D=%d H=%d W=%d", name, N, C, D, H, W);
    MVS_REQUIRE(K >= 1 && K <= MVSDET_MAX_NEIGHBORS, "%s: K=%d outside [1,%d]", name, K, MVSDET_MAX_NEIGHBORS);
    MVS_REQUIRE(gc_width_ok(C, G),
                "%s: C=%d G=%d: the group width C/G must divide C and be 4, 8, 16 or a multiple of 32 (C %% G == 0 and C/G in {4, 8, 16} "
                "or C/G %% 32 == 0)", name, C, G);
    MVS_REQUIRE(D <= MVSDET_MAX_DEPTH && H < 65535 && W < 65535, "%s: D > %d, or H or W > 65534", name, MVSDET_MAX_DEPTH);
    MVS_REQUIRE((size_t)H * W * kSlab * sizeof(float) < (size_t)INT32_MAX, "%s: one slab image exceeds 2^31 bytes", name);
    MVS_REQUIRE((size_t)D * H * W < (size_t)INT32_MAX, "%s: the depth hypotheses of one view exceed 2^31 elements", name);
    MVS_REQUIRE(ds[0] >= 0 && ds[1] >= 0 && ds[2] >= 0, "%s: negative depth stride", name);
    MVS_REQUIRE(N <= 65535 && num_slabs(C) <= 65535, "%s: N or C too large (N and the slab count must be <= 65535)", name);
    const long long tiles = ((long long)H * W + kTilePix - 1) / kTilePix;
    MVS_REQUIRE((long long)N * tiles * num_slabs(C) <= INT32_MAX / 2, "%s: grid too large", name);
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
    const int U = mode == kCgSlabs ? G : S;   // units: a group's slabs, or one slab of whole groups
    const int tiles = (HW + kTilePix - 1) / kTilePix;
    const int n_bt = N * tiles;
    long long grid_x = (long long)n_bt * U;
    int xcd_parts = 1;
    if (U < 8 && 8 % U == 0 && options().sweep_xcd != 0) {   // an XCD owns a unit (compacted for fewer than 8 units)
        xcd_parts = 8 / U;
        grid_x = 8LL * ((n_bt + xcd_parts - 1) / xcd_parts);
    }
    const int dpb = gc_d_per_block(grid_x, D, 4);
    MVS_REQUIRE((D + dpb - 1) / dpb <= 65535, "%s: grid too large", name);
    const int vec = (HW % 4 == 0) && ((uintptr_t)out % 16 == 0);
    const float inv_cg = 1.0f / (float)cg;
    dim3 grid((unsigned)grid_x, (unsigned)((D + dpb - 1) / dpb));
    hipStream_t st = (hipStream_t)stream;
    const long long ds_n = depth_strides[0], ds_d = depth_strides[1], ds_p = depth_strides[2];
#define MVS_GC_FWD(KV, MV)                                                                                                            \
    hipLaunchKernelGGL((plane_sweep_groupcorr_kernel<KV, MV>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, ds_n, ds_d, ds_p, \
                       out, N, G, S, SG, U, D, H, W, tiles, dpb, n_bt, xcd_parts, inv_cg, vec)
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
    const size_t pb = mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W);
    if (workspace_bytes < pb) {
        set_error("%s: workspace %zu B < %zu B", name, workspace_bytes, pb);
        return MVSDET_ERR_WORKSPACE;
    }
    MVS_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", name);
    hipStream_t st = (hipStream_t)stream;
    float* gpacked = static_cast<float*>(workspace);
    if (hipMemsetAsync(gpacked, 0, pb, st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", name);
        return MVSDET_ERR_HIP;
    }
    const int S = num_slabs(C), HW = H * W, cg = C / G;
    const int SG = cg >= kSlab ? cg / kSlab : 1, ngl = cg >= kSlab ? 1 : kSlab / cg;
    const int lg_shift = cg == 4 ? 2 : (cg == 8 ? 3 : (cg == 16 ? 4 : 5));
    const int tiles = (HW + kTilePix - 1) / kTilePix;
    const long long nblocks = (long long)N * tiles * S;
    const int dpb = gc_d_per_block(nblocks, D, 0);
    const float inv_cg = 1.0f / (float)cg;
    const long long ds_n = depth_strides[0], ds_d = depth_strides[1], ds_p = depth_strides[2];
    dim3 grid((unsigned)nblocks, (unsigned)((D + dpb - 1) / dpb));
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
    if (HW % 4 == 0 && (uintptr_t)gfeat % 16 == 0) {
        dim3 dgrid((HW + 127) / 128, S, N);
        hipLaunchKernelGGL(unpack_features_dense_kernel, dgrid, dim3(kThreads), 0, st, gpacked, gfeat, C, S, HW);
    } else {
        dim3 ugrid((HW + 63) / 64, S, N);
        hipLaunchKernelGGL(unpack_features_kernel, ugrid, dim3(kThreads), 0, st, gpacked, gfeat, C, S, H, W);
    }
    MVS_LAUNCH_CHECK("unpack_features");
    return MVSDET_OK;
}
