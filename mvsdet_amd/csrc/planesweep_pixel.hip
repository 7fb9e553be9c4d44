// The per-pixel form of stage 1: homo_warping with depth_values (B,D,H,W) (mvs_models/module.py:130-133) -- every
// reference pixel carries its own D depth hypotheses, what a coarse-to-fine cost volume sweeps -- as a compatibility warp
// (a3) and as the fused variance (a3+a4), each with its backward with respect to the features.  The sampling grid carries
// no gradient (module.py:115), so the depths get none.
//
// This is not a homography per plane: neighbouring pixels may sample anywhere along their epipolar lines, so nothing of the
// plane form's geometry (footprint boxes, runs of planes, kFlagInside, the table in the scratch buffer) applies, and
// sweep_kernel.h's kernels are untouched.  What IS shared is the arithmetic: sample_ray / sample_at / decode_sample /
// tap_weights of sweep_kernel.h and the rounding points of oracle/planesweep_oracle.c mode 1 (taps nw, ne, sw, se as one
// product and three fused multiply-adds; S = f + w_1 + .. + w_K; Q = fma(w_j, w_j, Q) from f*f; m = S*r, var = fma(-m, m,
// Q*r)).  A depth map that is constant per plane therefore gives the plane operators' results bit for bit.
//
// Forward, plane_sweep_variance_pixel_kernel: block = (reference view, 128 consecutive pixels of the flattened map, 32-channel
// slab), slab s dealt to XCD s as the plane kernel does (an XCD's L2 holds one 128-byte slab of every source texel).  Lanes
// are (pixel slot ps = lane >> 3, channel group g = lane & 7) and own 4 consecutive pixels x 4 channels (8i + g), so
//   * a tap is ONE 16-byte load per lane straight from the packed maps, the 8 lanes of a slot covering the texel's 128 bytes
//     (the plane kernel's arithmetic where a footprint does not fit its LDS box);
//   * a value leaves as 16 bytes per lane = 8 channel rows x 128 contiguous bytes per wave-instruction, non-temporal.  With
//     this lane map the transpose happens in the registers: the rows are whole without a trip through LDS;
//   * the decode duty is split over the 8 lanes of a slot: lane (ps, g) reads the depth (coalesced: the wave's 32
//     consecutive pixels) and decodes the position of pixel-step g & 3 for neighbour 2p + (g >> 2) in pass p -- one
//     position per lane, pass and hypothesis -- and the slot fetches offsets and weights with DPP.
//
// Backward, sweep_pixel_bwd_kernel: the same blocks; per hypothesis the block brings dL/dvar of its (slab, 128 pixels) through
// LDS (coalesced rows in, texel order out) and decodes every (neighbour, pixel) once into LDS; then lanes run over the 32
// floats of a slab texel, two pixels per wave-instruction, recompute the warped values, and scatter each tap gradient with
// atomicAdd(float*) into a packed gradient map in the workspace -- every atomic wave-instruction is two 128-byte texel
// segments (full rate on gfx950; one lane per row is an order of magnitude slower).  The reference view's own term is
// summed over the hypotheses in LDS and added once.  The packed gradient is then unpacked to (N,C,H,W) by pack.h's pass.
// Atomic sums depend on arrival order: the gradient may differ in the last bits from run to run.
// The compatibility warp's backward is the WARP instantiation: K = 1, no reference-view term, no source reads.
//
// Out of scope here: fp16 storage, pitched output, view shards and tabled / pooled geometry for the per-pixel form; LDS
// staging of footprints (or LDS gradient images) for smooth depth maps; an autograd formula for the (B,D) ops.homo_warp.
#include "common.h"

#include <algorithm>

#include "pack.h"
#include "sweep_kernel.h"

namespace mvsdet {

// a3, per-pixel: homo_warp_kernel (planesweep.hip) with the depth read per output pixel.
__global__ __launch_bounds__(kThreads) void homo_warp_pixel_kernel(const float* __restrict__ src, const float* __restrict__ proj,
                                                                    const float* __restrict__ depth, float* __restrict__ out, int C,
                                                                    int D, int H, int W) {
    const int HW = H * W;
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const int d = blockIdx.y, b = blockIdx.z;
    if (pix >= HW) return;
    const int y = pix / W, x = pix - y * W;
    int4 off;
    float4 w;
    compute_taps(proj + (size_t)b * 16, (float)x, (float)y, depth[((size_t)b * D + d) * HW + pix], H, W, 1, off, w);
    const float* plane = src + (size_t)b * C * HW;
    float* o = out + ((size_t)b * C * D + d) * HW + pix;
    for (int c = 0; c < C; ++c) {
        float s = plane[off.x] * w.x;
        s = fmaf(plane[off.y], w.y, s);
        s = fmaf(plane[off.z], w.z, s);
        s = fmaf(plane[off.w], w.w, s);
        *o = s;
        plane += HW;
        o += (size_t)D * HW;
    }
}

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

// block id -> (slab, view * tiles + tile): slab = id % S, or, for fewer than 8 slabs, an XCD owns a slab and takes one
// contiguous range of (view, tile) pairs (the plane kernel's dealing).  false: a padding block of the rounded-up grid.
__device__ __forceinline__ bool pixel_block(int id, int S, int n_bt, int xcd_parts, int& slab, int& bt) {
    slab = id % S;
    bt = id / S;
    if (xcd_parts > 1) {
        const int xcd = id & 7, k = id >> 3;
        const int per_part = (n_bt + xcd_parts - 1) / xcd_parts;
        slab = xcd % S;
        bt = (xcd / S) * per_part + k;
        if (k >= per_part) return false;
    }
    return bt < n_bt;
}

template <int K, bool FAST>
__global__ __launch_bounds__(kThreads) void plane_sweep_variance_pixel_kernel(
    const float* __restrict__ packed, const int64_t* __restrict__ nbr, const float* __restrict__ proj,
    const float* __restrict__ depth, float* __restrict__ var, int N, int C, int S, int D, int H, int W, int tiles, int d_per_block,
    int n_bt, int xcd_parts) {
    constexpr int KK = K > 0 ? K : 1;
    constexpr int NP = (K + 1) / 2;   // decode passes: a lane decodes ONE (pixel-step, neighbour) pair per pass
    constexpr int NPP = NP > 0 ? NP : 1;
    const int HW = H * W;
    int slab, bt;
    if (!pixel_block(blockIdx.x, S, n_bt, xcd_parts, slab, bt)) return;
    const int tile = bt % tiles, n = bt / tiles;
    const int d_begin = blockIdx.y * d_per_block, d_end = min(D, d_begin + d_per_block);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane & 7, ps = lane >> 3;
    const size_t slab_stride = (size_t)HW * kSlab;
    const float* ref_img = packed + ((size_t)n * S + slab) * slab_stride;
    const char* nb_img[KK];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int64_t v = nbr[(size_t)n * K + j];
        v = v < 0 ? 0 : (v >= N ? N - 1 : v);   // never read outside the packed maps (ids are validated on the host)
        nb_img[j] = reinterpret_cast<const char*>(packed + ((size_t)v * S + slab) * slab_stride);
    }
    const float rcp = 1.0f / (float)(K + 1);
    const int g16 = g * 16;   // the lane's 16 bytes of a texel

    // the lane's 4 consecutive pixels of the flattened map, their reference features (channels 8i + g) and squares
    const int p0 = tile * kTilePix + 32 * wave + 4 * ps;
    float f[4][4], fsq[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(ref_img + (size_t)min(p0 + s, HW - 1) * kSlab + 4 * g);
        f[s][0] = v.x; f[s][1] = v.y; f[s][2] = v.z; f[s][3] = v.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) fsq[s][i] = f[s][i] * f[s][i];
    }
    const int st_n = max(0, min(4, HW - p0));   // how many of the 4 pixels exist

    // decode duty: the pixel p0 + (g & 3), neighbour 2p + (g >> 2) in pass p
    const int qd = g >> 2;
    const int pd = p0 + (g & 3);
    const bool d_inside = pd < HW;
    const int pdc = min(pd, HW - 1);
    const int dy = pdc / W, dx = pdc - dy * W;
    SampleRay ray[NPP];
    float tr0[NPP], tr1[NPP], tr2[NPP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float* P = proj + ((size_t)n * K + min(2 * p + qd, K - 1)) * 16;
        ray[p] = sample_ray(P, (float)dx, (float)dy);
        tr0[p] = P[3]; tr1[p] = P[7]; tr2[p] = P[11];
    }
    const float* depth_px = K > 0 ? depth + (size_t)n * D * HW + pdc : nullptr;   // hypothesis d of the decoded pixel: + d * HW
    float dv_next = (K > 0 && d_begin < d_end) ? depth_px[(size_t)d_begin * HW] : 0.0f;

    for (int d = d_begin; d < d_end; ++d) {
        const float dval = dv_next;
        if (K > 0 && d + 1 < d_end) dv_next = depth_px[(size_t)(d + 1) * HW];   // requested a hypothesis ahead
        float Ssum[4][4], Qsum[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) { Ssum[s][i] = f[s][i]; Qsum[s][i] = fsq[s][i]; }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            // pixel outside the map: no tap inside, all weights +0 (nothing of it is stored)
            const float2 e_any = sample_at(ray[p], tr0[p], tr1[p], tr2[p], dval, H, W);
            const float2 e = d_inside ? e_any : make_float2(kNoSample, kNoSample);
            const SampleTaps tp = decode_sample(e.x, e.y, H, W);
            const float4 dw = tap_weights(tp);
            const int4 dof = tap_bytes(tp, H, W);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = 2 * p + q;
                if (j < K) {
                    const int ro0 = from_quad_sel(dof.x, q), ro1 = from_quad_sel(dof.y, q);
                    const int ro2 = from_quad_sel(dof.z, q), ro3 = from_quad_sel(dof.w, q);
                    const int rw0 = from_quad_sel(__float_as_int(dw.x), q), rw1 = from_quad_sel(__float_as_int(dw.y), q);
                    const int rw2 = from_quad_sel(__float_as_int(dw.z), q), rw3 = from_quad_sel(__float_as_int(dw.w), q);
                    float4 tq[4][4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {   // all 16 gathers of a neighbour requested ahead of their arithmetic
                        tq[s][0] = *reinterpret_cast<const float4*>(nb_img[j] + (quad_bcast_sel(ro0, s) + g16));
                        tq[s][1] = *reinterpret_cast<const float4*>(nb_img[j] + (quad_bcast_sel(ro1, s) + g16));
                        tq[s][2] = *reinterpret_cast<const float4*>(nb_img[j] + (quad_bcast_sel(ro2, s) + g16));
                        tq[s][3] = *reinterpret_cast<const float4*>(nb_img[j] + (quad_bcast_sel(ro3, s) + g16));
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float w0 = __int_as_float(quad_bcast_sel(rw0, s)), w1 = __int_as_float(quad_bcast_sel(rw1, s));
                        const float w2 = __int_as_float(quad_bcast_sel(rw2, s)), w3 = __int_as_float(quad_bcast_sel(rw3, s));
                        const float t0[4] = {tq[s][0].x, tq[s][0].y, tq[s][0].z, tq[s][0].w};
                        const float t1[4] = {tq[s][1].x, tq[s][1].y, tq[s][1].z, tq[s][1].w};
                        const float t2[4] = {tq[s][2].x, tq[s][2].y, tq[s][2].z, tq[s][2].w};
                        const float t3[4] = {tq[s][3].x, tq[s][3].y, tq[s][3].z, tq[s][3].w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float v = t0[i] * w0;
                            v = fmaf(t1[i], w1, v);
                            v = fmaf(t2[i], w2, v);
                            v = fmaf(t3[i], w3, v);
                            Ssum[s][i] = Ssum[s][i] + v;
                            Qsum[s][i] = fmaf(v, v, Qsum[s][i]);
                        }
                    }
                }
            }
        }
        // variance, and out: 16 bytes per lane = 8 channel rows x 128 contiguous bytes per wave-instruction, non-temporal
        // (written once, never re-read here: keeps the stream from evicting the source slabs)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float m = Ssum[s][i] * rcp;
                v[s] = fmaf(-m, m, Qsum[s][i] * rcp);
            }
            const int c = slab * kSlab + g + 8 * i;
            float* dst = var + (((size_t)n * C + c) * D + d) * HW + p0;
            if constexpr (FAST) {   // every channel row of the slab exists, the 4 pixels are all there or all not, 16-byte aligned
                if (st_n == 4) {
                    typedef float v4f __attribute__((ext_vector_type(4)));
                    const v4f vv = {v[0], v[1], v[2], v[3]};
                    __builtin_nontemporal_store(vv, reinterpret_cast<v4f*>(dst));
                }
            } else if (c < C) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s < st_n) dst[s] = v[s];
            }
        }
    }
}

// Backward of the per-pixel variance (WARP = false) or of the per-pixel compatibility warp (WARP = true: K == 1, the
// "neighbour" of batch row n is row n itself, dL/dwarped = g, no reference-view term and no source reads).
//   var = Q r - (S r)^2, r = 1/(K+1):  dvar/dv = 2 v r - 2 S r^2 = 2 r (v - m)  for every value v in {f, w_1..w_K}
//   w_j = sum_t weight_t tap_t  ->  dL/dtap_t += weight_t dL/dw_j, for the taps INSIDE the source map (zero padding)
template <int K, bool WARP>
__global__ __launch_bounds__(kThreads) void sweep_pixel_bwd_kernel(const float* __restrict__ packed, const int64_t* __restrict__ nbr,
                                                                    const float* __restrict__ proj, const float* __restrict__ depth,
                                                                    const float* __restrict__ gvar, float* __restrict__ gpacked, int N,
                                                                    int C, int S, int D, int H, int W, int tiles, int d_per_block) {
    constexpr int KK = K > 0 ? K : 1;
    constexpr int kPitch = kTilePix + 1;
    __shared__ float s_g[kSlab * kPitch];      // dL/dvar of hypothesis d: [channel of the slab][pixel of the tile]
    __shared__ int4 s_off[KK * kTilePix];      // element offsets of the 4 taps inside a slab image (clamped into it)
    __shared__ float4 s_w[KK * kTilePix];      // their weights (outside taps: weight * 0)
    __shared__ unsigned s_in[KK * kTilePix];   // bit t: tap t lies inside the source map
    __shared__ float s_ref[WARP ? 1 : kTilePix * kSlab];   // the reference view's own term, summed over the hypotheses
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
    const bool c_ok = slab * kSlab + crow < C;
    const float* ref_img = WARP ? nullptr : packed + ((size_t)n * S + slab) * slab_stride + q;
    const float* nb_img[KK];
    float* nb_grad[KK];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int64_t v = WARP ? (int64_t)n : nbr[(size_t)n * K + j];
        v = v < 0 ? 0 : (v >= N ? N - 1 : v);
        nb_img[j] = WARP ? nullptr : packed + ((size_t)v * S + slab) * slab_stride + q;
        nb_grad[j] = gpacked + ((size_t)v * S + slab) * slab_stride + q;
    }
    const float rcp = 1.0f / (float)(K + 1), two_r = 2.0f * rcp;
    if constexpr (!WARP) {
#pragma unroll
        for (int it = 0; it < 16; ++it) s_ref[(32 * wave + 2 * it + hw) * kSlab + q] = 0.0f;   // the lane's own cells throughout
    }
    for (int d = d_begin; d < d_end; ++d) {
        __syncthreads();   // every wave is done with the previous hypothesis' tables
        {   // dL/dvar: thread = (pixel of the tile, 16 channel rows): 512 contiguous bytes per row
            const int pl = tid & (kTilePix - 1), pix = pix0 + pl;
            for (int r = tid >> 7; r < kSlab; r += 2) {
                const int c = slab * kSlab + r;
                float v = 0.0f;
                if (pix < HW && c < C) v = gvar[(((size_t)n * C + c) * D + d) * HW + pix];
                s_g[r * kPitch + pl] = v;
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
                const float2 e = sample_at(r, P[3], P[7], P[11], depth[((size_t)n * D + d) * HW + pix], H, W);
                const SampleTaps tp = decode_sample(e.x, e.y, H, W);
                w = tap_weights(tp);
                const int4 b = tap_bytes(tp, H, W);
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
            const float go = s_g[crow * kPitch + pl];
            float coef[KK];
            if constexpr (WARP) {
                coef[0] = go;
            } else {
                const float fv = ref_img[(size_t)pix * kSlab];
                float vj[KK];
                float sum = fv;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int4 off = s_off[j * kTilePix + pl];
                    const float4 w = s_w[j * kTilePix + pl];
                    float v = nb_img[j][off.x] * w.x;
                    v = fmaf(nb_img[j][off.y], w.y, v);
                    v = fmaf(nb_img[j][off.z], w.z, v);
                    v = fmaf(nb_img[j][off.w], w.w, v);
                    vj[j] = v;
                    sum = sum + v;
                }
                const float m = sum * rcp, gs = go * two_r;
                s_ref[pl * kSlab + q] += gs * (fv - m);
#pragma unroll
                for (int j = 0; j < K; ++j) coef[j] = gs * (vj[j] - m);
            }
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
    if constexpr (!WARP) {
        float* ref_grad = gpacked + ((size_t)n * S + slab) * slab_stride + q;
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int pl = 32 * wave + 2 * it + hw, pix = pix0 + pl;
            if (pix < HW && c_ok && d_begin < d_end) atomicAdd(ref_grad + (size_t)pix * kSlab, s_ref[pl * kSlab + q]);
        }
    }
}

}  // namespace mvsdet

using namespace mvsdet;

namespace {

// hypotheses per block: all of them unless the grid would be too small to fill the chip
int pixel_d_per_block(long long nblocks, int D, int at_most) {
    int dsplit = 1;
    while (nblocks * dsplit < 2048 && dsplit < D) dsplit *= 2;
    dsplit = std::min(dsplit, D);
    int dpb = (D + dsplit - 1) / dsplit;
    if (at_most > 0) dpb = std::min(dpb, at_most);
    return dpb;
}

int pixel_shape_check(const char* name, int N, int K, int C, int D, int H, int W) {
    MVS_REQUIRE(N > 0 && C > 0 && D > 0 && H > 1 && W > 1, "%s: bad shape N=%d C=%d D=%d H=%d W=%d", name, N, C, D, H, W);
    MVS_REQUIRE(K >= 0 && K <= MVSDET_MAX_NEIGHBORS, "%s: K=%d outside [0,%d]", name, K, MVSDET_MAX_NEIGHBORS);
    MVS_REQUIRE(D <= MVSDET_MAX_DEPTH && H < 65535 && W < 65535, "%s: D > %d, or H or W > 65534", name, MVSDET_MAX_DEPTH);
    MVS_REQUIRE((size_t)H * W * kSlab * sizeof(float) < (size_t)INT32_MAX, "%s: one slab image exceeds 2^31 bytes", name);
    MVS_REQUIRE((size_t)D * H * W < (size_t)INT32_MAX, "%s: the depth hypotheses of one view exceed 2^31 elements", name);
    const long long tiles = ((long long)H * W + kTilePix - 1) / kTilePix;
    MVS_REQUIRE((long long)N * tiles * num_slabs(C) <= INT32_MAX / 2, "%s: grid too large", name);
    return MVSDET_OK;
}

int pixel_unpack(const float* gpacked, float* gfeat, int N, int C, int H, int W, hipStream_t stream) {
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

template <bool WARP>
int pixel_bwd_launch(const char* name, const float* packed, const int64_t* nbr, const float* proj, const float* depth, const float* g,
                     float* gfeat, void* workspace, size_t workspace_bytes, int N, int K, int C, int D, int H, int W, hipStream_t stream) {
    const size_t pb = mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W);
    if (workspace_bytes < pb) {
        set_error("%s: workspace %zu B < %zu B", name, workspace_bytes, pb);
        return MVSDET_ERR_WORKSPACE;
    }
    MVS_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", name);
    MVS_REQUIRE(N <= 65535 && num_slabs(C) <= 65535, "%s: N or C too large", name);
    float* gpacked = static_cast<float*>(workspace);
    if (hipMemsetAsync(gpacked, 0, pb, stream) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", name);
        return MVSDET_ERR_HIP;
    }
    const int S = num_slabs(C);
    const int tiles = (H * W + kTilePix - 1) / kTilePix;
    const long long nblocks = (long long)N * tiles * S;
    const int dpb = pixel_d_per_block(nblocks, D, 0);
    dim3 grid((unsigned)nblocks, (unsigned)((D + dpb - 1) / dpb));
#define MVS_PIXEL_BWD(KV)                                                                                                       \
    case KV:                                                                                                                    \
        hipLaunchKernelGGL((sweep_pixel_bwd_kernel<KV, WARP>), grid, dim3(kThreads), 0, stream, packed, nbr, proj, depth, g, gpacked, \
                           N, C, S, D, H, W, tiles, dpb);                                                                       \
        break;
    if constexpr (WARP) {
        switch (K) { MVS_PIXEL_BWD(1) }
    } else {
        switch (K) {
            MVS_PIXEL_BWD(0)
            MVS_PIXEL_BWD(1)
            MVS_PIXEL_BWD(2)
            MVS_PIXEL_BWD(3)
            MVS_PIXEL_BWD(4)
        }
    }
#undef MVS_PIXEL_BWD
    MVS_LAUNCH_CHECK(name);
    return pixel_unpack(gpacked, gfeat, N, C, H, W, stream);
}

}  // namespace

extern "C" int mvsdet_homo_warp_pixel_f32(const float* src, const float* proj, const float* depth, float* out, int B, int C, int D,
                                          int H, int W, mvsdet_stream_t stream) {
    MVS_REQUIRE(src && proj && depth && out, "homo_warp_pixel: NULL pointer");
    MVS_REQUIRE(B > 0 && C > 0 && D > 0 && H > 1 && W > 1, "homo_warp_pixel: bad shape B=%d C=%d D=%d H=%d W=%d", B, C, D, H, W);
    MVS_REQUIRE(B <= 65535 && D <= 65535, "homo_warp_pixel: B or D > 65535");
    MVS_REQUIRE((size_t)C * H * W < (size_t)INT32_MAX, "homo_warp_pixel: one view exceeds 2^31 elements");
    MVS_REQUIRE((size_t)D * H * W < (size_t)INT32_MAX, "homo_warp_pixel: the depth hypotheses of one view exceed 2^31 elements");
    dim3 grid((H * W + kThreads - 1) / kThreads, D, B);
    hipLaunchKernelGGL(homo_warp_pixel_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, src, proj, depth, out, C, D, H, W);
    MVS_LAUNCH_CHECK("homo_warp_pixel");
    return MVSDET_OK;
}

extern "C" int mvsdet_plane_sweep_variance_pixel_packed_f32(const float* packed, const int64_t* nbr, const float* proj,
                                                            const float* depth, float* var, int N, int K, int C, int D, int H, int W,
                                                            mvsdet_stream_t stream) {
    const char* name = "plane_sweep_variance_pixel";
    MVS_REQUIRE(packed && var, "%s: NULL pointer", name);
    MVS_REQUIRE(K == 0 || (nbr && proj && depth), "%s: NULL neighbour ids / proj / depth with K=%d", name, K);
    if (int rc = pixel_shape_check(name, N, K, C, D, H, W)) return rc;
    const int S = num_slabs(C), HW = H * W;
    const int tiles = (HW + kTilePix - 1) / kTilePix;
    const int n_bt = N * tiles;
    long long grid_x = (long long)n_bt * S;
    int xcd_parts = 1;
    if (S < 8 && 8 % S == 0 && options().sweep_xcd != 0) {   // an XCD owns a slab (compacted for fewer than 8 slabs)
        xcd_parts = 8 / S;
        grid_x = 8LL * ((n_bt + xcd_parts - 1) / xcd_parts);
    }
    const int dpb = pixel_d_per_block(grid_x, D, 4);
    MVS_REQUIRE((D + dpb - 1) / dpb <= 65535, "%s: grid too large", name);
    const bool fast = (C % kSlab == 0) && (HW % 4 == 0) && ((uintptr_t)var % 16 == 0);
    dim3 grid((unsigned)grid_x, (unsigned)((D + dpb - 1) / dpb));
    hipStream_t st = (hipStream_t)stream;
#define MVS_PIXEL_FWD(KV)                                                                                                          \
    case KV:                                                                                                                       \
        if (fast)                                                                                                                  \
            hipLaunchKernelGGL((plane_sweep_variance_pixel_kernel<KV, true>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, var, \
                               N, C, S, D, H, W, tiles, dpb, n_bt, xcd_parts);                                                     \
        else                                                                                                                       \
            hipLaunchKernelGGL((plane_sweep_variance_pixel_kernel<KV, false>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, var, \
                               N, C, S, D, H, W, tiles, dpb, n_bt, xcd_parts);                                                     \
        break;
    switch (K) {
        MVS_PIXEL_FWD(0)
        MVS_PIXEL_FWD(1)
        MVS_PIXEL_FWD(2)
        MVS_PIXEL_FWD(3)
        MVS_PIXEL_FWD(4)
    }
#undef MVS_PIXEL_FWD
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

// the packed gradient map, rounded up to 256 bytes
extern "C" size_t mvsdet_plane_sweep_pixel_bwd_workspace_bytes(int N, int C, int H, int W) {
    return (mvsdet_packed_bytes(N, C, H, W) + 255) / 256 * 256;
}

extern "C" int mvsdet_plane_sweep_variance_pixel_bwd_packed_f32(const float* packed, const int64_t* nbr, const float* proj,
                                                                const float* depth, const float* g, float* gfeat, void* workspace,
                                                                size_t workspace_bytes, int N, int K, int C, int D, int H, int W,
                                                                mvsdet_stream_t stream) {
    const char* name = "plane_sweep_variance_pixel_bwd";
    MVS_REQUIRE(packed && g && gfeat && workspace, "%s: NULL pointer", name);
    MVS_REQUIRE(K == 0 || (nbr && proj && depth), "%s: NULL neighbour ids / proj / depth with K=%d", name, K);
    if (int rc = pixel_shape_check(name, N, K, C, D, H, W)) return rc;
    return pixel_bwd_launch<false>(name, packed, nbr, proj, depth, g, gfeat, workspace, workspace_bytes, N, K, C, D, H, W,
                                   (hipStream_t)stream);
}

extern "C" int mvsdet_homo_warp_pixel_bwd_f32(const float* proj, const float* depth, const float* g, float* gsrc, void* workspace,
                                              size_t workspace_bytes, int B, int C, int D, int H, int W, mvsdet_stream_t stream) {
    const char* name = "homo_warp_pixel_bwd";
    MVS_REQUIRE(proj && depth && g && gsrc && workspace, "%s: NULL pointer", name);
    if (int rc = pixel_shape_check(name, B, 1, C, D, H, W)) return rc;
    return pixel_bwd_launch<true>(name, nullptr, nullptr, proj, depth, g, gsrc, workspace, workspace_bytes, B, 1, C, D, H, W,
                                  (hipStream_t)stream);
}
