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
// Blocks, lanes, the decode, the gathers and tap sums of the forward, and the decode into LDS, the recomputed warped value, the
// atomic scatter and the reference view's own term of the backward are the per-pixel form's shared steps: pixel_form.h, which
// groupcorr.hip uses too.  What is this file's own:
//
// Forward, plane_sweep_variance_pixel_kernel: a block's unit is one 32-channel slab, slab s dealt to XCD s as the plane kernel
// does (an XCD's L2 holds one 128-byte slab of every source texel); the depth is read contiguous (coalesced: the wave's 32
// consecutive pixels), a hypothesis ahead; S and Q are summed per value as the tap sums arrive; a value leaves as 16 bytes per
// lane = 8 channel rows x 128 contiguous bytes per wave-instruction, non-temporal.  With the shared lane map the transpose
// happens in the registers: the rows are whole without a trip through LDS.
//
// Backward, sweep_pixel_bwd_kernel: per hypothesis the block brings dL/dvar of its (slab, 128 pixels) through LDS (coalesced rows
// in, texel order out); the coefficient of a value v in {f, w_1..w_K} is 2 r (v - m) dL/dvar.
// The compatibility warp's backward is the WARP instantiation: K = 1, no reference-view term, no source reads.
//
// Out of scope here: fp16 storage, pitched output, view shards and tabled / pooled geometry for the per-pixel form; LDS
// staging of footprints (or LDS gradient images) for smooth depth maps; an autograd formula for the (B,D) ops.homo_warp.
#include "pixel_form.h"

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

template <int K, bool FAST>
__global__ __launch_bounds__(kThreads) void plane_sweep_variance_pixel_kernel(
    const float* __restrict__ packed, const int64_t* __restrict__ nbr, const float* __restrict__ proj,
    const float* __restrict__ depth, float* __restrict__ var, int N, int C, int S, int D, int H, int W, int tiles, int d_per_block,
    int n_bt, int xcd_parts) {
    constexpr int KK = K > 0 ? K : 1;
    const int HW = H * W;
    int slab, bt;
    if (!pixel_block(blockIdx.x, S, n_bt, xcd_parts, slab, bt)) return;
    const int tile = bt % tiles, n = bt / tiles;
    const int d_begin = blockIdx.y * d_per_block, d_end = min(D, d_begin + d_per_block);
    const size_t slab_stride = (size_t)HW * kSlab;
    const float* ref_img = packed + ((size_t)n * S + slab) * slab_stride;
    const char* nb_img[KK];
#pragma unroll
    for (int j = 0; j < K; ++j) nb_img[j] = reinterpret_cast<const char*>(packed + (neighbour_view(nbr, n, K, j, N) * S + slab) * slab_stride);
    const float rcp = 1.0f / (float)(K + 1);
    const PixelLanes L = pixel_lanes(tile, HW);
    const int g = L.g, p0 = L.p0, st_n = L.st_n;

    // the lane's reference features (channels 8i + g) of its 4 pixels and their squares
    float f[4][4], fsq[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(ref_img + (size_t)min(p0 + s, HW - 1) * kSlab + 4 * g);
        f[s][0] = v.x; f[s][1] = v.y; f[s][2] = v.z; f[s][3] = v.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) fsq[s][i] = f[s][i] * f[s][i];
    }
    const DecodeDuty<K> dd = decode_duty<K>(L, proj, n, H, W);
    const float* depth_px = K > 0 ? depth + (size_t)n * D * HW + dd.pdc : nullptr;   // hypothesis d of the decoded pixel: + d * HW
    float dv_next = (K > 0 && d_begin < d_end) ? depth_px[(size_t)d_begin * HW] : 0.0f;

    for (int d = d_begin; d < d_end; ++d) {
        const float dval = dv_next;
        if (K > 0 && d + 1 < d_end) dv_next = depth_px[(size_t)(d + 1) * HW];   // requested a hypothesis ahead
        int ro[KK][4], rw[KK][4];
        pixel_decode<K>(dd, dval, H, W, ro, rw);
        float Ssum[4][4], Qsum[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) { Ssum[s][i] = f[s][i]; Qsum[s][i] = fsq[s][i]; }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float4 tq[4][4];
            gather_4x4(nb_img[j], ro[j], L.g16, tq);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float w[4];
                step_weights(rw[j], s, w);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = warped_value(tq[s], w, i);
                    Ssum[s][i] = Ssum[s][i] + v;
                    Qsum[s][i] = fmaf(v, v, Qsum[s][i]);
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
    __shared__ TapTables<KK> s_tap;
    __shared__ float s_ref[WARP ? 1 : kTilePix * kSlab];   // the reference view's own term, summed over the hypotheses
    const int HW = H * W;
    const PixelBwdBlock b = pixel_bwd_block(C, S, D, HW, tiles, d_per_block);
    const int n = b.n, tid = b.tid;
    const float* ref_img = WARP ? nullptr : packed + b.img + b.q;
    const float* nb_img[KK];
    float* nb_grad[KK];
    pixel_bwd_neighbours<K, WARP>(b, packed, gpacked, nbr, N, S, HW, nb_img, nb_grad);
    const float rcp = 1.0f / (float)(K + 1), two_r = 2.0f * rcp;
    if constexpr (!WARP) pixel_bwd_ref_zero(b, s_ref);
    for (int d = b.d_begin; d < b.d_end; ++d) {
        __syncthreads();   // every wave is done with the previous hypothesis' tables
        {   // dL/dvar: thread = (pixel of the tile, 16 channel rows): 512 contiguous bytes per row
            const int pl = tid & (kTilePix - 1), pix = b.pix0 + pl;
            for (int r = tid >> 7; r < kSlab; r += 2) {
                const int c = b.slab * kSlab + r;
                float v = 0.0f;
                if (pix < HW && c < C) v = gvar[(((size_t)n * C + c) * D + d) * HW + pix];
                s_g[r * kPitch + pl] = v;
            }
        }
        pixel_bwd_decode<K>(b, proj, depth + ((size_t)n * D + d) * HW, 1, H, W, s_tap);
        __syncthreads();
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int pl = pixel_bwd_pl(b, it), pix = b.pix0 + pl;
            if (pix >= HW) continue;
            const float go = s_g[b.crow * kPitch + pl];
            float coef[KK];
            if constexpr (WARP) {
                coef[0] = go;
            } else {
                const float fv = ref_img[(size_t)pix * kSlab];
                float vj[KK];
                float sum = fv;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    vj[j] = tap_sum(nb_img[j], s_tap.off[j * kTilePix + pl], s_tap.w[j * kTilePix + pl]);
                    sum = sum + vj[j];
                }
                const float m = sum * rcp, gs = go * two_r;
                s_ref[pl * kSlab + b.q] += gs * (fv - m);
#pragma unroll
                for (int j = 0; j < K; ++j) coef[j] = gs * (vj[j] - m);
            }
            if (b.c_ok) {
#pragma unroll
                for (int j = 0; j < K; ++j)
                    tap_scatter(nb_grad[j], s_tap.off[j * kTilePix + pl], s_tap.w[j * kTilePix + pl], s_tap.in[j * kTilePix + pl], coef[j]);
            }
        }
    }
    if constexpr (!WARP) pixel_bwd_ref_flush(b, s_ref, gpacked, HW);
}

}  // namespace mvsdet

using namespace mvsdet;

namespace {

template <bool WARP>
int pixel_bwd_launch(const char* name, const float* packed, const int64_t* nbr, const float* proj, const float* depth, const float* g,
                     float* gfeat, void* workspace, size_t workspace_bytes, int N, int K, int C, int D, int H, int W, hipStream_t stream) {
    if (int rc = pixel_bwd_prologue(name, workspace, workspace_bytes, N, C, H, W, stream)) return rc;
    float* gpacked = static_cast<float*>(workspace);
    const int S = num_slabs(C);
    const PixelBlocking pb = pixel_blocking(N, C, 0, D, H, W, true);
    const int tiles = pb.tiles, dpb = pb.d_per_block;
    dim3 grid((unsigned)pb.grid_x, (unsigned)((D + dpb - 1) / dpb));
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
    if (int rc = pixel_shape_check(name, N, K, 0, C, D, H, W)) return rc;
    const int S = num_slabs(C), HW = H * W;
    const PixelBlocking pb = pixel_blocking(N, C, 0, D, H, W, false);   // an XCD owns a slab
    const int tiles = pb.tiles, n_bt = pb.n_bt, dpb = pb.d_per_block;
    MVS_REQUIRE((D + dpb - 1) / dpb <= 65535, "%s: grid too large", name);
    const bool fast = (C % kSlab == 0) && (HW % 4 == 0) && ((uintptr_t)var % 16 == 0);
    dim3 grid((unsigned)pb.grid_x, (unsigned)((D + dpb - 1) / dpb));
    hipStream_t st = (hipStream_t)stream;
#define MVS_PIXEL_FWD(KV)                                                                                                          \
    case KV:                                                                                                                       \
        if (fast)                                                                                                                  \
            hipLaunchKernelGGL((plane_sweep_variance_pixel_kernel<KV, true>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, var, \
                               N, C, S, D, H, W, tiles, dpb, n_bt, pb.xcd_parts);                                                    \
        else                                                                                                                       \
            hipLaunchKernelGGL((plane_sweep_variance_pixel_kernel<KV, false>), grid, dim3(kThreads), 0, st, packed, nbr, proj, depth, var, \
                               N, C, S, D, H, W, tiles, dpb, n_bt, pb.xcd_parts);                                                    \
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

// HOST query: how the per-pixel form cuts this problem into blocks under the options in force -- pixel_blocking, what the launches
// themselves call.  Nothing is launched.
extern "C" int mvsdet_pixel_form_blocking(int N, int C, int G, int D, int H, int W, int backward, int* units, int* xcd_parts,
                                          int* d_per_block) {
    const char* name = "pixel_form_blocking";
    MVS_REQUIRE(units && xcd_parts && d_per_block, "%s: NULL pointer", name);
    if (int rc = pixel_shape_check(name, N, 1, 0, C, D, H, W)) return rc;
    MVS_REQUIRE(G >= 0, "%s: G=%d is negative (0: variance / warp, G > 0: group correlation)", name, G);
    MVS_REQUIRE(G == 0 || gc_width_ok(C, G),
                "%s: C=%d G=%d: the group width C/G must divide C and be 4, 8, 16 or a multiple of 32", name, C, G);
    const PixelBlocking pb = pixel_blocking(N, C, G, D, H, W, backward != 0);
    *units = pb.units;
    *xcd_parts = pb.xcd_parts;
    *d_per_block = pb.d_per_block;
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
    if (int rc = pixel_shape_check(name, N, K, 0, C, D, H, W)) return rc;
    return pixel_bwd_launch<false>(name, packed, nbr, proj, depth, g, gfeat, workspace, workspace_bytes, N, K, C, D, H, W,
                                   (hipStream_t)stream);
}

extern "C" int mvsdet_homo_warp_pixel_bwd_f32(const float* proj, const float* depth, const float* g, float* gsrc, void* workspace,
                                              size_t workspace_bytes, int B, int C, int D, int H, int W, mvsdet_stream_t stream) {
    const char* name = "homo_warp_pixel_bwd";
    MVS_REQUIRE(proj && depth && g && gsrc && workspace, "%s: NULL pointer", name);
    if (int rc = pixel_shape_check(name, B, 1, 0, C, D, H, W)) return rc;
    return pixel_bwd_launch<true>(name, nullptr, nullptr, proj, depth, g, gsrc, workspace, workspace_bytes, B, 1, C, D, H, W,
                                  (hipStream_t)stream);
}
