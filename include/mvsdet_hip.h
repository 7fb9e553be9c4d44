/*
 * mvsdet_hip.h -- C ABI of the MI355X (gfx950) plane-sweep hot path of MVSDet.
 *
 * This is the drop-in boundary.  The reference has no FFI on this path: it
 * is Python calling PyTorch operators.  Each entry point below replaces a
 * block of reference Python (file:line relative to projects/NeRF-Det/nerfdet/ of Pixie8888/MVSDet)
 * and is what a maintainer would bind from that Python with ctypes (INTEGRATION.md shows the
 * stub).  mvsdet_amd/_lib.py is exactly such a binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.cuda tensor storage) unless marked HOST;
 *   - tensors are fp32, dense row-major in the stated shape unless a stride array is given
 *     (strides are in ELEMENTS, HOST arrays of 4 int64);
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work: no allocation, no
 *     host synchronisation, so they can be captured in a hipGraph;
 *   - return 0 on success, an MVSDET_ERR_* code otherwise; mvsdet_last_error() (HOST, thread-local)
 *     describes the failure.  Nothing is launched when an argument check fails.
 */
#ifndef MVSDET_HIP_H
#define MVSDET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVSDET_OK 0
#define MVSDET_ERR_INVALID_ARG 1 /* bad shape / NULL pointer / unsupported size */
#define MVSDET_ERR_WORKSPACE 2   /* workspace too small */
#define MVSDET_ERR_HIP 3         /* a HIP runtime call failed (launch error) */

#define MVSDET_MAX_NEIGHBORS 4 /* k source views per reference view (reference: k = min(2, N-1)) */
#define MVSDET_MAX_TOPK 8      /* depth candidates per pixel (reference: topk = 3) */
#define MVSDET_MAX_DEPTH 512   /* depth planes (reference: 12; BASELINE configs go to 128) */

typedef void* mvsdet_stream_t; /* hipStream_t */

/* ABI version: major*1000 + minor. */
int mvsdet_version(void);
/* HOST, thread-local message of the last failing call on this thread ("" if none). */
const char* mvsdet_last_error(void);
/* Tuning options (schedule only: results are bit-identical under every setting).  Read ONCE from the environment
 * (MVSDET_SWEEP_TW, MVSDET_SWEEP_BOXCAP, MVSDET_SWEEP_XCD) when the library first needs them,
 * afterwards changed only through mvsdet_set_option -- the launch path never calls getenv.  HOST, process-global:
 * set them before launching from several threads.
 *   "sweep_tw"      0 (by the map shape) | 16 | 32   pixel-tile shape of the sweep (16x8 / 32x4)
 *   "sweep_boxcap"  texels of one LDS footprint box (default: what fits, 312 / 200 by the tile shape; 0 = gather every tap
 *                   from global memory)
 *   "sweep_xcd"     0 | 1   XCD-aware block map for fewer than 8 channel slabs
 *   "sweep_inside"  1 (default) | 0   planes whose bilinear taps all lie inside the source image take the slab kernel's lean
 *                   decode (no range tests, no clamps of the tap offsets); 0 = every plane takes the general decode
 *   "sweep_pool"    1 (default) | 0   mvsdet_plane_sweep_table_pooled_f32 builds the pooled geometry; 0 = it builds what
 *                   mvsdet_plane_sweep_table[_pitched]_f32 build
 *   "sweep_store"   0 (default) = non-temporal | 1 plain | 2 sc1 | 3 sc0 sc1 | 4 nt sc1   cache policy of the sweep's output stores
 *                   (FAST form, two neighbours) and of mvsdet_store_pattern_probe_*; MVSDET_SWEEP_STORE.  A value selects a compiled
 *                   instantiation: the default build carries 0 alone, the A/B build (make SWEEP_STORE_MATRIX=1) all of them, and
 *                   mvsdet_set_option refuses a value that is not compiled in
 *   "sweep_box_load"  0 (default) | 1 = non-temporal   cache policy of the footprint boxes' LDS-DMA and of a block's reference-feature
 *                   loads; MVSDET_SWEEP_BOX_LOAD; compiled and refused like "sweep_store"
 *   "depthprob_ahead"  1 (default) | 0  mvsdet_depth_prob_topk[_strided]_f32 requests every input of a pixel before its first
 *                   store (D <= 64), or runs its last pass eight planes ahead (D > 64); 0 = plane by plane, behind the stores
 *   "pixel_dsplit"  0 (default: by the grid size) | n > 0   the per-pixel form's blocks walk ceil(D / min(n, D)) consecutive depth hypotheses
 *                   each, the forwards at most 4 (mvsdet_pixel_form_blocking shows the outcome); MVSDET_PIXEL_DSPLIT
 *   "sweep_dsplit", "sweep_groups", "bwd_groups", "conv_*"   schedules of the sweep's plane split, of the bf16x3
 *                   convolutions and of the fp16 + MX convolution ("conv_mx_th") (csrc/common.h: struct Options)
 * "sweep_tw" decides the layout of the sweep geometry: consume one (mvsdet_plane_sweep_variance_tabled_f32) under the
 * "sweep_tw" it was built with (mvsdet_plane_sweep_table_f32).  "sweep_boxcap" is baked into the geometry (union boxes,
 * staged / refill flags); the consuming call sizes its LDS slots for the largest capacity a geometry of that tile shape
 * can carry, so "sweep_boxcap", "sweep_xcd" and "sweep_inside" may change between the two calls. */
int mvsdet_set_option(const char* name /*HOST*/, int value);
int mvsdet_get_option(const char* name /*HOST*/, int* value /*HOST*/);
/* HOST check of neighbour view ids before they are uploaded (mvsdet.py:434 feeds them to an index gather, where an
 * id outside [0, n_src) raises): MVSDET_ERR_INVALID_ARG names the first offending entry.  The kernels additionally
 * clamp ids, so a tensor that never passed through this check cannot make them read outside the packed maps. */
int mvsdet_validate_neighbors(const int64_t* nbr /*HOST (M,K)*/, int M, int K, int n_src);

/* ---------------------------------------------------------------------------------------------
 * Packed feature maps.
 * The sweep and the fused voxel lifting read 2-D features channel-last so that one bilinear tap /
 * one voxel sample is a single contiguous run of all channels.  Packed layout:
 *     packed[n][s][y][x][q],  s in [0, S), S = ceil(C/32) channel slabs,  q in [0, 32),
 *     q = 4*g + i  <->  channel c = 32*s + 8*i + g      (g in [0,8), i in [0,4))
 * (zero where c >= C): one texel of one slab is one 128-byte line, and every slab of a view is a
 * contiguous H*W*128-byte image.  mvsdet_packed_bytes() = N*S*H*W*32*sizeof(float).
 * mvsdet_pack_features_f32 reads element (n,c,y,x) at feat[n*fs[0] + c*fs[1] + y*fs[2] + x*fs[3]],
 * so the reference's non-contiguous crop feature[:, :, :h, :w] (mvsdet.py:499) needs no copy.
 * ------------------------------------------------------------------------------------------- */
size_t mvsdet_packed_bytes(int N, int C, int H, int W);
int mvsdet_pack_features_f32(const float* feat, const int64_t* feat_strides /*HOST[4]*/, float* packed,
                             int N, int C, int H, int W, mvsdet_stream_t stream);
/* Same for IEEE binary16 feature maps (BASELINE configs[4], `--amp` style fp16 features): element strides of the
 * half tensor; the packed maps are fp32 (conversion is exact), so every consumer below is unchanged. */
int mvsdet_pack_features_f16(const void* feat_f16, const int64_t* feat_strides /*HOST[4]*/, float* packed,
                             int N, int C, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a3  homo_warping -- mvs_models/module.py:105-146.
 *   src  (B,C,H,W)   source-view features
 *   proj (B,4,4)     src_proj @ inverse(ref_proj)  (module.py:116; computed by the caller with the
 *                    same torch ops as the reference -- see DESIGN.md "geometry stays on the host")
 *   depth(B,D)       plane depths
 *   out  (B,C,D,H,W) warped features: bilinear, zero padding, align_corners=False sampling of a grid
 *                    normalised with the align_corners=True formula (module.py:137-143), no z>0 test.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_homo_warp_f32(const float* src, const float* proj, const float* depth, float* out,
                         int B, int C, int D, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a3+a4  plane-sweep variance cost volume -- mvsdet.py:439-467 (k calls of homo_warping fused with
 * the running sum / sum of squares and the variance).
 *   packed (see above) features of all N views; nbr (N,K) int64 neighbour view ids (mvsdet.py:434);
 *   proj (N,K,4,4) = nei_proj[n][j] @ inverse(ref_proj[n]);  depth (N,D);
 *   var (N,C,D,H,W) = sum_sq/(K+1) - (sum/(K+1))^2 over {ref, warped_1..K}  (mvsdet.py:467).
 * `scratch` (16-byte aligned, >= mvsdet_plane_sweep_scratch_bytes(N,K,D,H,W)) receives the
 * channel-independent sweep geometry the sweep builds first: per (view, 128-pixel tile, plane,
 * neighbour) the footprint box that the sweep keeps resident in LDS -- shared by runs of
 * consecutive planes (sweep_kernel.h) --, one flags word per (view, tile, plane), and copies of
 * proj / depth: 20 B per (view, tile, plane) and neighbour, 0.03 % of the cost volume.  The sample
 * positions themselves are recomputed by the sweep (the reference builds its grid per plane too).
 * The _f32 form packs `feat` (N,C,H,W dense) into `workspace` first
 * (workspace_bytes >= mvsdet_plane_sweep_workspace_bytes(N,K,C,D,H,W) = packed + scratch).
 * ------------------------------------------------------------------------------------------- */
/* The pixel-tile shape (32x4 or 16x8) and the LDS box capacity in texels the sweep uses for this problem; the layout of
 * the geometry at the head of the scratch buffer follows from them: boxes int4[N][tiles][D][K], then flags
 * uint32[N][tiles][D], tiles = ceil(W / tile_w) * ceil(H / tile_h).  For tools and statistics (bench.py). */
int mvsdet_plane_sweep_tile_shape(int K, int D, int H, int W, int* tile_w, int* tile_h, int* box_texels);
size_t mvsdet_plane_sweep_scratch_bytes(int N, int K, int D, int H, int W);
size_t mvsdet_plane_sweep_workspace_bytes(int N, int K, int C, int D, int H, int W);
int mvsdet_plane_sweep_variance_packed_f32(const float* packed, const int64_t* nbr, const float* proj,
                                           const float* depth, float* var, void* scratch,
                                           size_t scratch_bytes, int N, int K, int C, int D, int H, int W,
                                           mvsdet_stream_t stream);
/* View shard of the same sweep (intra-scene split): the M reference views ref_first .. ref_first+M-1
 * of a scene whose N_src views are ALL in `packed` (neighbours are arbitrary views).  nbr (M,K) holds GLOBAL view
 * ids; nbr, proj (M,K,4,4), depth (M,D), var (M,C,D,H,W) and scratch (sized for M views) are indexed by the local
 * view.  Row m of the result is bit-identical to row ref_first+m of the unsharded call. */
int mvsdet_plane_sweep_variance_shard_f32(const float* packed, const int64_t* nbr, const float* proj,
                                          const float* depth, float* var, void* scratch, size_t scratch_bytes,
                                          int N_src, int ref_first, int M, int K, int C, int D, int H, int W,
                                          mvsdet_stream_t stream);
/* fp16 storage of the cost volume: identical fp32 arithmetic, var_f16 (M,C,D,H,W) IEEE binary16 = the fp32 result
 * rounded to nearest-even at the store (values above 65504 become +inf).  Halves the write stream, which is 96 % of
 * the sweep's bytes; with view shards it is how the 100-view / 128-plane / 240x320 configuration fits in HBM. */
int mvsdet_plane_sweep_variance_shard_f16(const float* packed, const int64_t* nbr, const float* proj,
                                          const float* depth, void* var_f16, void* scratch, size_t scratch_bytes,
                                          int N_src, int ref_first, int M, int K, int C, int D, int H, int W,
                                          mvsdet_stream_t stream);
/* The two halves of the call above, for callers that want to time / overlap / reuse them (the geometry of a scene can
 * be built once and swept with any number of feature sets):
 *   mvsdet_plane_sweep_table_f32           builds the sweep geometry of a scene's cameras into `scratch`;
 *   mvsdet_plane_sweep_variance_tabled_f32 runs the per-channel sweep on a geometry built by it for the SAME
 *                                          (N,K,D,H,W) (table_bytes = the scratch size passed there). */
int mvsdet_plane_sweep_table_f32(const float* proj, const float* depth, void* scratch, size_t scratch_bytes,
                                 int N, int K, int D, int H, int W, mvsdet_stream_t stream);
int mvsdet_plane_sweep_variance_tabled_f32(const float* packed, const int64_t* nbr, const void* table,
                                           size_t table_bytes, float* var, int N, int K, int C, int D, int H,
                                           int W, mvsdet_stream_t stream);
/* fp16 storage of the tabled sweep: the values mvsdet_plane_sweep_variance_shard_f16 stores, var_f16 (N,C,D,H,W) contiguous. */
int mvsdet_plane_sweep_variance_tabled_f16(const float* packed, const int64_t* nbr, const void* table,
                                           size_t table_bytes, void* var_f16, int N, int K, int C, int D, int H,
                                           int W, mvsdet_stream_t stream);
/* The same two calls for a PITCHED cost volume: `var` is (N,C,D,H,out_w_pitch) in memory and columns [0, W) of every row are
 * written (the caller hands out that view; mvsdet.py:467 materialises a contiguous volume -- same values, other strides).
 * With out_w_pitch a multiple of 32 every row starts on a 128-byte line and the sweep writes whole lines from 32x4 pixel
 * tiles even when W is no multiple of 32 (the 80-wide maps of the shipped configs: 64-byte runs otherwise).  The geometry
 * must be built with the pitch it is consumed with. */
int mvsdet_plane_sweep_table_pitched_f32(const float* proj, const float* depth, void* scratch, size_t scratch_bytes, int N,
                                         int K, int D, int H, int W, int out_w_pitch, mvsdet_stream_t stream);
/* The geometry under the POOLED run policy, for the forward sweep: with K == 2 and 32x4 pixel tiles the two LDS slots of a
 * block are one pool, and over planes on which one neighbour has no footprint the other's union box may take up to
 * 2 * (capacity + 8) - 8 texels at the pool's base -- fewer box refills on the near planes, the same results bit for bit.
 * Every other (K, tile shape) gets the slot geometry.  The table carries its own mark: mvsdet_plane_sweep_variance_tabled_f32
 * and _tabled_pitched_f32 take it (build it with the out_w_pitch it is consumed with; 0 or W = contiguous), the backward
 * (mvsdet_plane_sweep_variance_bwd_packed_f32) refuses it like any mismatched geometry: NaN output, nothing touched. */
int mvsdet_plane_sweep_table_pooled_f32(const float* proj, const float* depth, void* scratch, size_t scratch_bytes, int N,
                                        int K, int D, int H, int W, int out_w_pitch, mvsdet_stream_t stream);
int mvsdet_plane_sweep_variance_tabled_pitched_f32(const float* packed, const int64_t* nbr, const void* table,
                                                   size_t table_bytes, float* var, int N, int K, int C, int D, int H, int W,
                                                   int out_w_pitch, mvsdet_stream_t stream);
int mvsdet_plane_sweep_variance_f32(const float* feat, const int64_t* nbr, const float* proj,
                                    const float* depth, float* var, void* workspace, size_t workspace_bytes,
                                    int N, int K, int C, int D, int H, int W, mvsdet_stream_t stream);
/* backward of the above w.r.t. feat (the sampling grid carries no gradient, module.py:115).
 *   g (N,C,D,H,W) = dL/dvar;  gfeat (N,C,H,W) is OVERWRITTEN with dL/dfeat.
 *   workspace_bytes >= mvsdet_plane_sweep_bwd_workspace_bytes(N,K,C,D,H,W)
 *   (packed features + packed gradient + sweep geometry). */
size_t mvsdet_plane_sweep_bwd_workspace_bytes(int N, int K, int C, int D, int H, int W);
int mvsdet_plane_sweep_variance_bwd_f32(const float* feat, const int64_t* nbr, const float* proj,
                                        const float* depth, const float* g, float* gfeat, void* workspace,
                                        size_t workspace_bytes, int N, int K, int C, int D, int H, int W,
                                        mvsdet_stream_t stream);
/* The same from what the forward pass already made (a training step keeps them instead of making them again): `packed` =
 * mvsdet_pack_features_f32 of the features, `table` = the scratch buffer the forward call
 * (mvsdet_plane_sweep_variance_packed_f32 / mvsdet_plane_sweep_table_f32, same N, K, D, H, W and tile options; contiguous, not
 * pitched) left its sweep geometry in.  workspace >= mvsdet_packed_bytes(N,C,H,W) rounded up to 256 (the packed gradient map). */
int mvsdet_plane_sweep_variance_bwd_packed_f32(const float* packed, const int64_t* nbr, const void* table, size_t table_bytes,
                                               const float* g, float* gfeat, void* workspace, size_t workspace_bytes, int N, int K,
                                               int C, int D, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a3 / a3+a4 at PER-PIXEL depth hypotheses -- homo_warping's depth_values (B,D,H,W) form (mvs_models/module.py:130-133):
 * every reference pixel carries its own D hypotheses (what a coarse-to-fine cost volume sweeps).  Same sampling and the
 * same rounding points as the plane forms above: a depth map that is constant per plane gives their results bit for bit.
 * No geometry scratch.  The depths carry no gradient (the grid is built under no_grad, module.py:115).
 *   depth (B,D,H,W) / (N,D,H,W) contiguous;  out (B,C,D,H,W);  var (N,C,D,H,W) contiguous fp32;  K in [0, MVSDET_MAX_NEIGHBORS].
 * Backward passes: g = dL/dout resp. dL/dvar, contiguous; gsrc (B,C,H,W) / gfeat (N,C,H,W) are OVERWRITTEN.  The tap
 * gradients are summed with float atomics into a packed gradient map in `workspace` (>=
 * mvsdet_plane_sweep_pixel_bwd_workspace_bytes, 16-byte aligned, overwritten), so the last bits depend on arrival order.
 * Not offered in this form: fp16 storage, pitched output, view shards, tabled / pooled geometry.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_homo_warp_pixel_f32(const float* src, const float* proj, const float* depth, float* out,
                               int B, int C, int D, int H, int W, mvsdet_stream_t stream);
int mvsdet_homo_warp_pixel_bwd_f32(const float* proj, const float* depth, const float* g, float* gsrc, void* workspace,
                                   size_t workspace_bytes, int B, int C, int D, int H, int W, mvsdet_stream_t stream);
int mvsdet_plane_sweep_variance_pixel_packed_f32(const float* packed, const int64_t* nbr, const float* proj, const float* depth,
                                                 float* var, int N, int K, int C, int D, int H, int W, mvsdet_stream_t stream);
size_t mvsdet_plane_sweep_pixel_bwd_workspace_bytes(int N, int C, int H, int W);
int mvsdet_plane_sweep_variance_pixel_bwd_packed_f32(const float* packed, const int64_t* nbr, const float* proj,
                                                     const float* depth, const float* g, float* gfeat, void* workspace,
                                                     size_t workspace_bytes, int N, int K, int C, int D, int H, int W,
                                                     mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Group-wise correlation cost volume (the reference's mvs_models/lss_fpn.py:499-506), fused with the warp:
 *   out[n,j,g,d,y,x] = (1/Cg) * sum over the Cg = C/G channels c of group g of  f[n,c,y,x] * warped_j[n,c,d,y,x]
 * out (N,K,G,D,H,W) contiguous fp32, one volume per neighbour j; warped_j is what mvsdet_homo_warp[_pixel]_f32 returns for
 * the view nbr[n,j] (same sampling, zero padding, NaN for a non-finite position); group g = channels [g*Cg, (g+1)*Cg).
 *   packed: the packed maps of all N views;  nbr (N,K) int64, K in [1, MVSDET_MAX_NEIGHBORS] (a view may be its own
 *   neighbour, a neighbour may repeat);  proj (N,K,4,4).
 *   depth + depth_strides[3] = {view, hypothesis, pixel} in elements, all >= 0: hypothesis d of pixel p of view n is
 *   depth[n*s0 + d*s1 + p*s2], p = y*W + x.  (N,D,H,W) contiguous: {D*H*W, H*W, 1};  plane depths (N,D): {D, 1, 0}.
 *   Group widths: C % G == 0 and Cg in {4, 8, 16} or Cg % 32 == 0; anything else is MVSDET_ERR_INVALID_ARG.  With Cg in
 *   {4, 8, 16} C need not be a multiple of 32.  One slab image < 2^31 bytes; N and the slab count <= 65535.
 * The forward uses no atomics: the same inputs give the same bits on every run.
 * Backward: grad = dL/dout (N,K,G,D,H,W) contiguous; gfeat (N,C,H,W) is OVERWRITTEN with dL/dfeat (the reference view's own
 * term and the neighbours' tap gradients; depth and proj get none).  The tap gradients are summed with float atomics into a
 * packed gradient map in `workspace` (>= mvsdet_plane_sweep_pixel_bwd_workspace_bytes(N, C, H, W), 16-byte aligned,
 * overwritten): the last bits depend on arrival order.  MVSDET_ERR_WORKSPACE for a workspace that is too small.
 * Not offered: fp16 storage, pitched output, view shards.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_plane_sweep_groupcorr_packed_f32(const float* packed, const int64_t* nbr, const float* proj, const float* depth,
                                            const int64_t* depth_strides, float* out, int N, int K, int C, int G, int D, int H,
                                            int W, mvsdet_stream_t stream);
int mvsdet_plane_sweep_groupcorr_bwd_packed_f32(const float* packed, const int64_t* nbr, const float* proj, const float* depth,
                                                const int64_t* depth_strides, const float* grad, float* gfeat, void* workspace,
                                                size_t workspace_bytes, int N, int K, int C, int G, int D, int H, int W,
                                                mvsdet_stream_t stream);
/* HOST query, nothing is launched: how the per-pixel form above (variance, compatibility warp's backward, group correlation and its
 * backward) cuts a problem into blocks under the options in force -- the very function the launches call.  G = 0: variance / warp;
 * G > 0: group correlation with G groups.  backward != 0: the backward launch.
 *   units        what blocks are dealt over: 32-channel slabs, or for group widths that are multiples of 32 the G groups
 *   xcd_parts    1, or 8 / units where an XCD owns a unit (forward, units in {1, 2, 4}, "sweep_xcd" != 0)
 *   d_per_block  consecutive depth hypotheses a block walks (the forward: at most 4); the last block of a (view, tile, unit) may walk fewer
 * Shapes and group widths are checked as by the entry points (MVSDET_ERR_INVALID_ARG).  For tests and tools. */
int mvsdet_pixel_form_blocking(int N, int C, int G, int D, int H, int W, int backward, int* units /*HOST*/, int* xcd_parts /*HOST*/,
                               int* d_per_block /*HOST*/);

/* ---------------------------------------------------------------------------------------------
 * a5-a7  depth probability, top-k plane selection, depth expectation --
 * mvsdet.py:470-475 (softmax / sigmoid), :266-283 (sample_depth_prob), :298-317 (compute_avg_depth).
 *   cost_reg, off_logit (N,D,H,W)  the two output channels of CostRegNet_3DGS
 *   prob, off (N,D,H,W)            softmax over D / sigmoid
 *   est_depth, est_dens (N,topk,H,W) the topk most probable planes, descending; depth =
 *                                  idx*interval + near + off[idx]*interval; dens = prob[idx] (raw)
 *   est_idx (N,topk,H,W) int32     chosen plane indices (may be NULL); ties -> lower index
 *   avg_depth (N,H,W)              sum_d prob_d * (d*interval + near + off_d*interval)
 * ------------------------------------------------------------------------------------------- */
int mvsdet_depth_prob_topk_f32(const float* cost_reg, const float* off_logit, float* prob, float* off,
                               float* est_depth, float* est_dens, int32_t* est_idx, float* avg_depth,
                               int N, int D, int H, int W, int topk, float near, float interval,
                               mvsdet_stream_t stream);
/* The same with the two inputs as channel slices of the network's (N, 2, D, H, W) output (mvsdet.py:469 torch.unbind):
 * view n of either input starts view_stride floats after view n-1, its (D, H, W) block is dense.  Saves the two copies
 * that making the slices contiguous costs. */
int mvsdet_depth_prob_topk_strided_f32(const float* cost_reg, const float* off_logit, long long view_stride, float* prob,
                                       float* off, float* est_depth, float* est_dens, int32_t* est_idx, float* avg_depth,
                                       int N, int D, int H, int W, int topk, float near, float interval,
                                       mvsdet_stream_t stream);
/* a6+a7 only, for callers that already hold prob = softmax(cost_reg) and off = sigmoid(off_logit)
 * (signature-level parity with MVSDet.sample_depth_prob / compute_avg_depth, mvsdet.py:266,298). */
int mvsdet_sample_depth_prob_f32(const float* prob, const float* off, float* est_depth, float* est_dens,
                                 int32_t* est_idx, float* avg_depth, int N, int D, int H, int W, int topk,
                                 float near, float interval, mvsdet_stream_t stream);
/* NVS-branch input -- mvsdet.py:1158-1216 compute_depth_scale / compute_depth_scale_MultiIntrin and :494:
 *   intr (N,5) = {fx, fy, cx, cy, skew} of the feature-level intrinsics of every view (K[:2] / ratio, mvsdet.py:1180-1181);
 *   depth_scale (N,h,w) = z component of the normalised camera ray through pixel (x, y) (lift :1300 + normalize :1295);
 *   est_ray_depth (N,J,h,w) = est_depth[:, :, :h, :w] / (depth_scale + 1e-8), est_depth (N,J,H,W) padded maps (both NULL to
 *   get the scale alone). */
int mvsdet_ray_depth_f32(const float* intr, const float* est_depth, float* depth_scale, float* est_ray_depth, int N, int J,
                         int H, int W, int h, int w, mvsdet_stream_t stream);
/* backward: any of g_prob (N,D,H,W), g_depth, g_dens (N,topk,H,W), g_avg (N,H,W) may be NULL. */
int mvsdet_depth_prob_topk_bwd_f32(const float* prob, const float* off, const int32_t* est_idx,
                                   const float* g_prob, const float* g_depth, const float* g_dens,
                                   const float* g_avg, float* g_cost, float* g_offlogit, int N, int D,
                                   int H, int W, int topk, float near, float interval, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Head of the cost regularisation network (first step): mvs_models/mvsnet.py:102,112
 *   self.prob = nn.Conv3d(64, 2, 3, stride=1, padding=1);  x = self.prob(x)
 * x (N,Cin,D,H,W) dense fp32, weight (2,Cin,3,3,3), bias (2) or NULL -> out (N,2,D,H,W): the (cost, offset)
 * logits that mvsdet_depth_prob_topk_f32 consumes.  Forward only (training keeps the framework's convolution).
 * ------------------------------------------------------------------------------------------- */
/* The ConvBnReLU3D layers of the same network on the fp32 matrix cores (exact fp32 FMA sums): Conv3d k=3, padding 1, no bias,
 *   stride 1 (mvs_models/mvsnet.py:76,79,82: conv0 256->64, conv2 128->128, conv4 256->256): x (N,Cin,D,H,W) dense fp32 ->
 *            out (N,Cout,D,H,W);
 *   stride 2 (mvsnet.py:78,81: conv1 64->128, conv3 128->256): -> out (N,Cout,(D-1)/2+1,(H-1)/2+1,(W-1)/2+1).
 * Cout a multiple of 64.  weight_perm: the (Cout,Cin,3,3,3) weight permuted to [c][kd][kh][kw][o] (Cin rounded up to even, zero
 * padded), 16-byte aligned.  scale / shift (Cout each, or both NULL): out = v*scale[o] + shift[o] -- eval-mode BatchNorm folded;
 * relu != 0 clamps at 0.  residual (shape of out, or NULL; stride 1 only) is added between the affine and the ReLU:
 * out = act(v*scale[o] + shift[o] + residual) -- the tail of the 3-D neck's ResModule, mmdet3d/models/necks/imvoxel_neck.py:219-230
 * (x = conv1(conv0(x)); x = x + identity; x = relu(x)).  Forward only.
 * Small volumes (imvoxel_neck.py:183-231, the 3-D neck's residual blocks at one scene, and nerfdet_head.py:96-101, the head's
 * convolutions: 400 / 50 / 8 tiles of 256 voxels): with a workspace of mvsdet_conv3d_k3_mfma_workspace_bytes(...) bytes (0 = the
 * grid fills the chip unsplit) the input-channel loop is split over several blocks per tile, which write raw partial sums; a
 * second kernel adds them in ascending split order and applies affine, residual and ReLU.  workspace NULL or too small (0
 * bytes): unsplit. */
size_t mvsdet_conv3d_k3_mfma_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int stride);
int mvsdet_conv3d_k3_mfma_ws_f32(const float* x, const float* weight_perm, const float* scale, const float* shift,
                                 const float* residual, float* out, void* workspace, size_t workspace_bytes, int N, int Cin,
                                 int Cout, int D, int H, int W, int stride, int relu, mvsdet_stream_t stream);
/* The up-sampling layers (mvsnet.py:92-100,110-111: conv9 256->128, conv11 128->64): ConvTranspose3d(kernel 3, stride 2,
 * padding 1, output_padding 1, no bias) [+ affine + ReLU] [+ residual]: x (N,Cin,D,H,W) -> out (N,Cout,2D,2H,2W);
 * weight_perm: the (Cin,Cout,3,3,3) weight permuted to [c][kd][kh][kw][o]; residual (shape of out, or NULL) is added
 * AFTER the affine + ReLU (x = skip + conv(x)).  Four launches, one per output parity in (d, h); a lane writes the two w
 * parities as one float2 (out and residual 8-byte aligned). */
int mvsdet_convT3d_k3_s2_mfma_f32(const float* x, const float* weight_perm, const float* scale, const float* shift,
                                  const float* residual, float* out, int N, int Cin, int Cout, int D, int H, int W, int relu,
                                  mvsdet_stream_t stream);
/* Weight gradient of the stride-1 layers (training): dW[o][c][tap] = sum_voxels grad_out[n][o][v] * x[n][c][v + tap - 1]
 * on the fp32 matrix cores.  partial (nsplit,Cout,Cin,27) fp32 receives one partial sum per voxel split
 * (mvsdet_conv3d_k3_dw_partial_bytes); the caller adds them up (deterministic, no atomics).  The input gradient of
 * these layers is mvsdet_conv3d_k3_mfma_ws_f32 on grad_out with the weights transposed and flipped. */
size_t mvsdet_conv3d_k3_dw_partial_bytes(int Cin, int Cout, int nsplit);
int mvsdet_conv3d_k3_dw_mfma_f32(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                                 int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* The same sum on the bf16 matrix cores with three-term split operands (the arithmetic of mvsdet_conv3d_k3_bf16x3_io: both
 * fp32 tensors are cut into bf16 pieces on the way into the LDS, products accumulate in fp32; relative error of a product
 * 2^-16).  Same arguments and partial layout. */
int mvsdet_conv3d_k3_dw_bf16x3(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                               int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* The same for the stride-2 layers (mvsnet.py:77,80: conv1, conv3): x (N,Cin,D,H,W) with even D, H, W, grad_out
 * (N,Cout,D/2,H/2,W/2); dW[o][c][tap] = sum grad_out[n][o][v] * x[n][c][2v + tap - 1].  With the two tensors exchanged --
 * x := the layer's grad_out (fine), grad_out := the layer's input (coarse) -- the result is the (Cin,Cout,3,3,3) weight
 * gradient of the transposed layers (mvsnet.py:92-100: conv9, conv11).  Their input gradients are each other's forward:
 * dX of a stride-2 layer = mvsdet_convT3d_k3_s2_mfma_f32 on grad_out with the layer's own (Cout,Cin,3,3,3) weight read
 * as a transposed-convolution weight, dX of a transposed layer = mvsdet_conv3d_k3_mfma_ws_f32 (stride 2) likewise. */
int mvsdet_conv3d_k3_s2_dw_mfma_f32(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                                    int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* The same sum (either orientation) on the bf16 matrix cores with three-term split operands (csrc/costreg_dw_s2_bf16.hip:
 * blocks of 64 coarse x 16 fine channels on v_mfma_f32_16x16x32_bf16; the fine rows are de-interleaved along w while they
 * are cut into bf16 pieces, so that every tap's fragment is one aligned LDS read).  Same arguments and partial layout;
 * W a multiple of 8 (the rows of both tensors are read as float4), D and H even. */
int mvsdet_conv3d_k3_s2_dw_bf16x3(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                                  int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* Training-mode BatchNorm3d [+ ReLU] of the network's ConvBnReLU3D / Sequential(ConvTranspose3d, BatchNorm3d, ReLU) blocks
 * (mvs_models/module.py:26-37, mvsnet.py:92-100): batch statistics over (N, D, H, W) per channel (biased variance),
 * running statistics updated in place with `momentum` (unbiased variance, as torch.nn.BatchNorm3d; NULL = not tracked),
 * out = [relu](gamma * (x - mean) * invstd + beta) (gamma / beta NULL = 1 / 0); save_mean / save_invstd (C floats) are what
 * the backward needs.  x and out are (N, C, vol) contiguous, vol = D*H*W.  workspace: mvsdet_bn3d_workspace_bytes(C).
 * A residual tensor (N, C, vol; NULL = none) is added AFTER the activation: out = [relu](bn(x)) + residual, the
 * `skip + Sequential(ConvTranspose3d, BatchNorm3d, ReLU)(x)` of mvsnet.py:109-111 without a pass of its own.
 * Backward: grad_x, grad_gamma, grad_beta (the last two may be NULL) from x, grad_out and the saved statistics; the ReLU
 * mask is recomputed from x with the forward's arithmetic (the residual's gradient is grad_out itself). */
size_t mvsdet_bn3d_workspace_bytes(int C);
int mvsdet_bn3d_relu_train_fwd_res_f32(const float* x, const float* gamma, const float* beta, const float* residual,
                                       float* running_mean, float* running_var, float* out, float* save_mean, float* save_invstd,
                                       void* workspace, size_t workspace_bytes, int N, int C, long long vol, float momentum, float eps,
                                       int relu, mvsdet_stream_t stream);
/* The same with the statistics taken from partial sums a producing convolution left (mvsdet_conv3d_k3_bf16x3_stats): partial[c * parts
 * + i] = (sum, sum of squares) of (x - pivot[c]) of channel c over block i, double2; pivot as given to the producer (NULL = zeros);
 * the entries are added in a fixed order. */
int mvsdet_bn3d_relu_train_fwd_parts_f32(const float* x, const void* partial, size_t parts, const float* pivot, const float* gamma, const float* beta,
                                         const float* residual, float* running_mean, float* running_var, float* out, float* save_mean,
                                         float* save_invstd, void* workspace, size_t workspace_bytes, int N, int C, long long vol,
                                         float momentum, float eps, int relu, mvsdet_stream_t stream);
int mvsdet_bn3d_relu_bwd_f32(const float* x, const float* grad_out, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma,
                             float* grad_beta, void* workspace, size_t workspace_bytes, int N, int C, long long vol, int relu,
                             mvsdet_stream_t stream);
/* Training-mode BatchNorm3d with the residual added INSIDE the activation, the tail of the 3-D neck's ResModule
 * (mmdet3d/models/necks/imvoxel_neck.py:219-230: relu(bn(conv1(h)) + identity)):
 *   out = [relu](gamma * (x - mean) * invstd + beta + residual), residual (N, C, vol) required;
 * statistics from a pass over x (partial NULL) or from a producer's partial sums (partial / parts / pivot as in
 * mvsdet_bn3d_relu_train_fwd_parts_f32); running statistics, save_mean / save_invstd and workspace as above.
 * Backward: g' = grad_out * [out > 0] (relu; `out` = the forward's output) or grad_out; grad_residual = g' (may be NULL);
 * grad_x, grad_gamma, grad_beta (the last two may be NULL) as mvsdet_bn3d_relu_bwd_f32 with g' as the masked gradient. */
int mvsdet_bn3d_res_relu_train_fwd_f32(const float* x, const void* partial, size_t parts, const float* pivot, const float* gamma,
                                       const float* beta, const float* residual, float* running_mean, float* running_var, float* out,
                                       float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, int N, int C,
                                       long long vol, float momentum, float eps, int relu, mvsdet_stream_t stream);
int mvsdet_bn3d_res_relu_bwd_f32(const float* x, const float* out, const float* grad_out, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_invstd, float* grad_x, float* grad_gamma, float* grad_beta,
                                 float* grad_residual, void* workspace, size_t workspace_bytes, int N, int C, long long vol, int relu,
                                 mvsdet_stream_t stream);
int mvsdet_conv3d_k3_cout2_f32(const float* x, const float* weight, const float* bias, float* out, int N, int Cin,
                               int D, int H, int W, mvsdet_stream_t stream);
/* The same layer on the SUM of two tensors, x + x2 (x2 NULL: x alone), formed while the halo tiles are staged: mvsnet.py:111-112
 * `x = conv0 + self.conv11(x); x = self.prob(x)` without the skip addition in the transposed layer's epilogue (which then is a
 * pure store stream).  A second input needs W % 4 == 0 and 16-byte aligned tensors. */
int mvsdet_conv3d_k3_cout2_sum_f32(const float* x, const float* x2, const float* weight, const float* bias, float* out, int N,
                                   int Cin, int D, int H, int W, mvsdet_stream_t stream);

/* Backward of the head (training): grad_x (N,Cin,D,H,W) from grad_out (N,2,D,H,W) and weight (2,Cin,3,3,3); and the
 * weight gradient as partial (nsplit,2,Cin,27) sums (one per voxel split, added up by the caller). */
int mvsdet_conv3d_k3_cout2_dx_f32(const float* grad_out, const float* weight, float* grad_x, int N, int Cin, int D, int H,
                                  int W, mvsdet_stream_t stream);
int mvsdet_conv3d_k3_cout2_dw_f32(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                                  int N, int Cin, int D, int H, int W, mvsdet_stream_t stream);
/* The weight gradient on the bf16 matrix cores with three-term split operands (within ~1e-5 of the fp32 sums' scale): x streams
 * from global memory straight into the MFMA fragments, grad_out's 3 x 3 neighbouring rows are staged per x row.  nsplit = blocks =
 * rows of partial (nsplit,2,Cin,27); Cin in {16, 32, 64}, W % 4 == 0, 16-byte aligned tensors (else MVSDET_ERR_INVALID_ARG: use
 * the fp32 call). */
int mvsdet_conv3d_k3_cout2_dw_bf16x3(const float* x, const float* grad_out, float* partial, size_t partial_bytes, int nsplit,
                                     int N, int Cin, int D, int H, int W, mvsdet_stream_t stream);
/* 1 if the call above takes this (Cin, W) -- channel count, row width and the LDS of a row stage (W up to ~470 at Cin = 64) --,
 * else 0: then mvsdet_conv3d_k3_cout2_dw_f32 is the entry point to use. */
int mvsdet_conv3d_k3_cout2_dw_bf16x3_ok(int Cin, int W);

/* ---------------------------------------------------------------------------------------------
 * a9  backproject_Weigh -- mvsdet.py:1372-1492 (gt_depth=None).
 *   feat + feat_strides: (N,C,h,w) view of the 2-D features (crop allowed, see pack above)
 *   points (3,V) voxel coordinates from get_points (mvsdet.py:1316); projection (N,3,4)
 *   depth, dens + dd_strides: candidate j of pixel (y,x) of view i at
 *       ptr[i*s[0] + j*s[1] + y*s[2] + x*s[3]]   (the reference's (N,h*w,1,J) tensors are views of this)
 *   vz = voxel_size[-1]
 *   volume (N,C,V) fp32; valid (N,V) uint8 (1 = voxel is in view i's frustum AND inside the depth
 *   window of at least one candidate).  xi, yi (N,V) int32 rounded pixel coordinates may be NULL.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_backproject_weigh_f32(const float* feat, const int64_t* feat_strides /*HOST[4]*/, const float* points,
                                 const float* projection, const float* depth, const float* dens,
                                 const int64_t* dd_strides /*HOST[4]*/, float* volume, uint8_t* valid,
                                 int32_t* xi, int32_t* yi, int N, int C, int h, int w, int V, int J, float vz,
                                 mvsdet_stream_t stream);
/* a9+a10 fused: per-voxel mean over views, mvsdet.py:511-515.
 *   packed: packed features of the FULL (N,C,H,W) maps; only pixels y<h, x<w are addressed.
 *   mean (C,V) fp32 = sum_i volume_i / (count + 1e-8), 0 where count == 0; count (V) int32. */
int mvsdet_backproject_weigh_mean_packed_f32(const float* packed, const float* points, const float* projection,
                                             const float* depth, const float* dens,
                                             const int64_t* dd_strides /*HOST[4]*/, float* mean, int32_t* count,
                                             int N, int C, int H, int W, int h, int w, int V, int J, float vz,
                                             mvsdet_stream_t stream);
/* Same kernel without the division: sum (C,V) = sum_i volume_i over the N views handed in, count (V).  A rank that
 * owns a contiguous shard of the views passes packed / projection / depth / dens offset to its first view; the
 * ranks' sums and counts are then all-reduced and divided once (mvsdet_amd/parallel.py). */
int mvsdet_backproject_weigh_sum_packed_f32(const float* packed, const float* points, const float* projection,
                                            const float* depth, const float* dens,
                                            const int64_t* dd_strides /*HOST[4]*/, float* sum, int32_t* count,
                                            int N, int C, int H, int W, int h, int w, int V, int J, float vz,
                                            mvsdet_stream_t stream);
/* backward of a9 w.r.t. features and dens (depth carries no gradient).
 *   g (N,C,V); gfeat (N,C,h,w) dense and gdens (N,J,h,w) dense are OVERWRITTEN. */
int mvsdet_backproject_weigh_bwd_f32(const float* feat, const int64_t* feat_strides /*HOST[4]*/, const float* points,
                                     const float* projection, const float* depth, const float* dens,
                                     const int64_t* dd_strides /*HOST[4]*/, const float* g, float* gfeat,
                                     float* gdens, int N, int C, int h, int w, int V, int J, float vz,
                                     mvsdet_stream_t stream);
/* backward of a9+a10 (fused mean): g (C,V) = dL/dmean. */
int mvsdet_backproject_weigh_mean_bwd_f32(const float* feat, const int64_t* feat_strides /*HOST[4]*/,
                                          const float* points, const float* projection, const float* depth,
                                          const float* dens, const int64_t* dd_strides /*HOST[4]*/,
                                          const int32_t* count, const float* g, float* gfeat, float* gdens,
                                          int N, int C, int h, int w, int V, int J, float vz,
                                          mvsdet_stream_t stream);
/* a9 with ground-truth depth: the two scalars the gt_depth branch of backproject_Weigh returns (mvsdet.py:1435-1484)
 * and what they are made of.  The volume of a9 does not depend on gt_depth; call the functions above for it.
 *   points, projection, depth, dens + dd_strides, vz: as for a9
 *   depth_mean + dm_strides: (N,h,w) depth expectation, element strides of a 3-D view (a crop of the padded map)
 *   gt_depth + gt_strides:   (N,Hg,Wg) ground truth, any Hg, Wg >= 1, element strides of a 3-D view
 *   gt_depth is resized to (h,w) as ATen's upsample_bilinear2d(align_corners=False) does it in fp32 (:1437);
 *   mask = resized > 0 (NaN stays outside); gt_valid = original_valid & (z > g - vz) & (z < g + vz) (:1470)
 *   scalars  (2)   fp32  {gap_all, rmse}: gap_all = mean of gap_i over the views with a valid' voxel (:1464, :1484),
 *                        NaN when there is none (the reference divides by zero and raises); rmse = mean over the mask
 *                        of (depth_mean - g)^2 (no square root, :1445), NaN for an empty mask
 *   per_view (N,4) fp32  {gap_i (NaN for a skipped view), orig_gap, new_gap, n_reduce} (:1473-1479)
 *   sums     (N,6) fp64  {sum (gt_valid - weight)^2 over original_valid, n original_valid, n valid',
 *                        sum (depth_mean - g)^2 over the mask, n mask, n (gt_valid != valid')}: what a caller that
 *                        splits the views needs to add up
 *   gt_resized (N,h,w) fp32 or NULL
 * Every term is formed in fp32 as the reference forms it and added in float64, per wave, per block and over the blocks
 * in a fixed order without atomics: results are bit-identical from call to call.
 * workspace (16-byte aligned) >= the query below: the resized map and one partial per block. */
size_t mvsdet_depth_diagnostics_workspace_bytes(int N, int h, int w, int V);
int mvsdet_depth_diagnostics_f32(const float* points, const float* projection, const float* depth, const float* dens,
                                 const int64_t* dd_strides /*HOST[4]*/, const float* depth_mean,
                                 const int64_t* dm_strides /*HOST[3]*/, const float* gt_depth,
                                 const int64_t* gt_strides /*HOST[3]*/, float* scalars, float* per_view, double* sums,
                                 float* gt_resized, void* workspace, size_t workspace_bytes, int N, int h, int w, int V,
                                 int J, int Hg, int Wg, float vz, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth supervision (csrc/depthloss.hip): the reference's two masked depth objectives, one scene per call.
 *   kind MVSDET_DEPTH_LOSS_L1         MVSDet.depth_loss_func_new (mvsdet.py:893-915): gt (N,Hg,Wg), any Hg, Wg >= 1, is resized to
 *                                     (h,w) as ATen's upsample_bilinear2d(align_corners=False) does it in fp32; the mask is
 *                                     resized > 0 (NaN stays outside); the term |est - resized|; mask / mask_strides are ignored
 *   kind MVSDET_DEPTH_LOSS_SMOOTH_L1  mvsnet_loss (mvs_models/mvsnet.py:292-294): gt and mask are (N,h,w) (Hg = h, Wg = w); inside
 *                                     where mask > 0.5; the term 0.5 d^2 for |d| < 1, else |d| - 0.5, d = est - gt (beta = 1)
 *   est + est_strides: (N,h,w), element strides of a 3-D view (the crop of a padded map is read in place, and only inside
 *   the mask); gt, mask + strides likewise.
 *   loss (1) fp32 = sum of the terms / count, NaN for an empty mask (0 / 0, torch.mean of nothing); count (1) int32.
 * Terms are formed in fp32 and added in float64 per wave, per block and over the blocks in a fixed order without atomics:
 * results are bit-identical from call to call.  Two launches, no host synchronisation.
 * workspace (16-byte aligned) >= the query below: one 16-byte partial per block of 256 pixels.
 * Backward: grad (N,h,w) contiguous, written densely: 0 outside the mask; inside (g_loss / count) * sign(d) (l1; sign(0) = 0) or
 * (g_loss / count) * clamp(d, -1, 1) (smooth_l1), the quotient one IEEE fp32 division.  g_loss (1) fp32 and count (1) int32 are
 * DEVICE pointers (count as the forward wrote it).  The resized ground truth is formed again from gt.  One launch. */
#define MVSDET_DEPTH_LOSS_L1 0
#define MVSDET_DEPTH_LOSS_SMOOTH_L1 1
size_t mvsdet_depth_loss_workspace_bytes(int N, int h, int w);
int mvsdet_depth_loss_f32(const float* est, const int64_t* est_strides /*HOST[3]*/, const float* gt,
                          const int64_t* gt_strides /*HOST[3]*/, const float* mask, const int64_t* mask_strides /*HOST[3]*/,
                          float* loss, int32_t* count, void* workspace, size_t workspace_bytes, int N, int h, int w, int Hg,
                          int Wg, int kind, mvsdet_stream_t stream);
int mvsdet_depth_loss_bwd_f32(const float* est, const int64_t* est_strides /*HOST[3]*/, const float* gt,
                              const int64_t* gt_strides /*HOST[3]*/, const float* mask,
                              const int64_t* mask_strides /*HOST[3]*/, const float* g_loss, const int32_t* count, float* grad,
                              int N, int h, int w, int Hg, int Wg, int kind, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Photometric consistency (csrc/photoloss.hip): the reference's self-supervised depth objective, mvs_models/homography.py
 * (inverse_warping, _bilinear_sample, compute_reconstr_loss) and MVSDet.photometric_loss (mvsdet.py:845-874).  fp32, no atomics, no
 * host synchronisation; every result is bit-identical from call to call.
 *
 * mvsdet_photo_geometry_f32 (one launch): for pair b, the left view left_idx[b] and the right view right_idx[b] (DEVICE int64; NULL =
 *   view b), geo[b] (24 floats) = K_left^-1 (9, row-major), K_left [R_right R_left^T | t_right - R_rel t_left] (12, row-major 3x4),
 *   3 unused -- the LEFT intrinsics project into the right view, as the reference has it.  Formed in float64 from the fp32 cameras
 *   (the inverse by the adjugate) and rounded once.  ext_*: rows [R|t] of 4 floats, *_view_stride elements between views ((N,4,4): 16,
 *   the packed (B,2,3,4) cameras: 24); k_left: 3 rows k_row_stride apart, k_view_stride between views (0: one matrix for all).
 *   An index outside [0, n_left) / [0, n_right) gives a NaN geometry and reads nothing.
 * mvsdet_photo_warp_f32 (one launch, one thread per (b, y, x)): img (n_img,h,w,C) through img_strides {view, y, x, channel} and
 *   src_idx[b], depth (n_depth,h,w) through depth_strides and depth_idx[b] (DEVICE int64; NULL = b, then the count must be B);
 *   xg (w), yg (h): the pixel grid (linspace(-1,1,W) + 1) * 0.5 * (W-1) of the reference, fp32.  Per pixel, in the reference's fp32
 *   order: cam = (K^-1 [xg,yg,1]) depth, p = P [cam;1], x = p0 / (p2 + 1e-10), the round trip / (W-1) * 2 - 1, (. + 1) * (W-1) / 2,
 *   x0 = floor(x), x1 = x0 + 1; mask = x0 >= 0 && x1 <= W-1 && y0 >= 0 && y0 <= H-1 (on y0; NaN is outside); the four indices
 *   clamped, weights from the CLAMPED x1, y1: wa = (x1-x)(y1-y) on (y0,x0), wb = (x1-x)(1-(y1-y)) on (y1,x0), wc on (y0,x1), wd on
 *   (y1,x1).  warped (B,h,w,C) and mask (B,h,w) float 0/1, contiguous; outside the mask warped is that same (extrapolating) formula.
 *   An index outside its range gives NaN, mask 0, and reads nothing.
 * mvsdet_photo_warp_bwd_f32 (one launch): grad (n_depth,h,w) contiguous, dense = sum over the pairs b with depth_idx[b] = view, in
 *   ascending b, of sum_c g_warped * d warped / d depth (floor and clamp carry no gradient).  A pixel whose g_warped is 0 in every
 *   channel contributes exactly 0.
 * mvsdet_photo_loss_f32 (two launches): wm = warped * mask, rm = ref * mask (ref (B,h,w,C) through ref_strides);
 *   terms[0] = mean smooth_l1(wm - rm) (beta 1), terms[1] / terms[2] = the same of the forward differences along w / h (each over its
 *   own B h (w-1) C / B (h-1) w C elements); loss (1) = simple ? terms[0] : 0.5 terms[0] + 0.5 (terms[1] + terms[2]); count (1) int32 = pixels
 *   with mask != 0.  Terms fp32, sums float64 per wave, per block, over the blocks in ascending order.
 *   workspace (16-byte aligned) >= the query: one 32-byte partial per block of 256 pixels.
 * mvsdet_photo_loss_bwd_f32 (one launch): grad (B,h,w,C) = g_loss (DEVICE) * d L / d warped, exactly 0 where mask = 0.
 * mvsdet_photo_select_f32 (two launches): masks (n, total) contiguous, L (n), n <= 32: per pixel v_i = L_i + 1e4 (1 - mask_i); the
 *   scene of the smallest v wins it (the lower index on a tie) if that v < 1e4.  wins (n) int32, loss (1) = sum_i wins_i L_i / total
 *   (float64, rounded once).  workspace >= the query.  mvsdet_photo_select_bwd_f32: grad (n) = g_loss (DEVICE) * wins_i / total. */
int mvsdet_photo_geometry_f32(const float* ext_left, int64_t ext_left_view_stride, const float* k_left, int64_t k_view_stride,
                              int64_t k_row_stride, const float* ext_right, int64_t ext_right_view_stride, const int64_t* left_idx,
                              const int64_t* right_idx, int n_left, int n_right, float* geo, int B, mvsdet_stream_t stream);
int mvsdet_photo_warp_f32(const float* img, const int64_t* img_strides /*HOST[4]*/, const int64_t* src_idx, int n_img,
                          const float* depth, const int64_t* depth_strides /*HOST[3]*/, const int64_t* depth_idx, int n_depth,
                          const float* geo, const float* xg, const float* yg, float* warped, float* mask, int B, int h, int w, int C,
                          mvsdet_stream_t stream);
int mvsdet_photo_warp_bwd_f32(const float* img, const int64_t* img_strides /*HOST[4]*/, const int64_t* src_idx, int n_img,
                              const float* depth, const int64_t* depth_strides /*HOST[3]*/, const int64_t* depth_idx, int n_depth,
                              const float* geo, const float* xg, const float* yg, const float* g_warped, float* grad, int B, int h,
                              int w, int C, mvsdet_stream_t stream);
size_t mvsdet_photo_loss_workspace_bytes(int B, int h, int w);
int mvsdet_photo_loss_f32(const float* warped, const float* mask, const float* ref, const int64_t* ref_strides /*HOST[4]*/, float* loss,
                          float* terms, int32_t* count, void* workspace, size_t workspace_bytes, int B, int h, int w, int C, int simple,
                          mvsdet_stream_t stream);
int mvsdet_photo_loss_bwd_f32(const float* warped, const float* mask, const float* ref, const int64_t* ref_strides /*HOST[4]*/,
                              const float* g_loss, float* grad, int B, int h, int w, int C, int simple, mvsdet_stream_t stream);
size_t mvsdet_photo_select_workspace_bytes(int n, int total);
int mvsdet_photo_select_f32(const float* masks, const float* L, int32_t* wins, float* loss, void* workspace, size_t workspace_bytes,
                            int n, int total, mvsdet_stream_t stream);
int mvsdet_photo_select_bwd_f32(const int32_t* wins, const float* g_loss, float* grad, int n, int total, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian rasteriser (csrc/splat.hip): what gs_src/model/decoder/cuda_splatting.py::render_cuda asks of its external extension
 * (Kerbl et al. 2023 with spherical harmonics up to degree 4), for V views that share one set of G Gaussians.  fp32, 16x16 tiles, no
 * float atomics, no host synchronisation; forward and backward are bit-identical from call to call.  DESIGN.md 4.15 has every
 * constant.  Limits: d_sh in {1, 4, 9, 16, 25}; V <= 65535; V G, V tiles, 9 V max_keys (10 with depth) and 3 V H W below 2^31.
 *
 * mvsdet_splat_cameras_f32 (one launch, one thread per view): cams (V,40) = view matrix (16) and full projection (16), both in the
 *   row-vector (transposed) form render_cuda hands over, tan(fov_x / 2), tan(fov_y / 2), camera position (3), scale, 2 unused -- from
 *   extrinsics (camera-to-world rows of 4 floats, ext_view_stride elements between views, last row taken as 0 0 0 1), normalised
 *   intrinsics (3 rows k_row_stride apart, k_view_stride between views) and near / far (V).  scale_invariant: scale = 1 / near
 *   multiplies the translation, near and far in fp32 as the reference does, and the rasteriser multiplies means by scale and
 *   covariances by scale^2 itself; otherwise scale = 1.  Inverses, field of view and the matrix product in float64, rounded once.
 * mvsdet_splat_forward_f32 and mvsdet_splat_backward_f32 are the one call form of every render; with_colour and with_depth choose
 *   what is blended: colour alone (1, 0), colour and depth in one pass (1, 1), depth alone (0, 1).  Both 0 is refused first.
 *   Always: means (G,3) through means_strides {g, c}, covariances (G,3,3) through cov_strides {g, row, col} (the upper triangle is
 *   read), opacities (G) opacity_stride apart, cams from above.  max_keys: (Gaussian, tile) pairs a view may have; the count a view
 *   needs goes to its status word, the first int4 block of the workspace {needed, capacity, overflow, 0} per view.  A view that needs
 *   more writes nothing past its share: its outputs are NaN and the backward gives NaN for every gradient.  workspace (256-byte
 *   aligned) >= the query, the same for every form; the backward reads it.
 *   With colour: harmonics (G,3,d_sh) through sh_strides {g, channel, k}, background (V,3) -> image (V,3,H,W) contiguous.  use_sh 0:
 *   harmonics (G,3,1) are the colours themselves (no basis, no + 0.5, no clamp).  The image has the same bits with and without depth.
 *   Without colour harmonics, sh_strides, background, image, g_image and g_harmonics are not touched and may be NULL; d_sh and use_sh
 *   are ignored.
 *   With depth (render_depth_cuda, cuda_splatting.py:237-280, as a fourth blended channel of the same pass): every
 *   (view, Gaussian) gets one value d = f(z), z its camera-space depth before the scale_invariant scaling, near / far (V) the caller's
 *   unscaled bounds: mode 0 depth z, 1 disparity 1 / z, 2 relative_disparity (conversions.py:17-27, eps 1e-10), 3 log as the reference
 *   writes it, log(max(min(z, near), far)) = log(far) whenever near <= far.  values (V,G) receives d (0 where culled), depth (V,H,W)
 *   the blend sum d alpha T over a background of 0, with the alpha, T, skips and early stop of the colour.  Without depth near, far,
 *   depth, values and g_depth are not touched and may be NULL, and mode is ignored.
 * mvsdet_splat_backward_f32 (two launches): g_image (V,3,H,W) and g_depth (V,H,W), contiguous, as the flags say -> g_means (G,3),
 *   g_covariances (G,3,3: upper triangle, the off-diagonals with both symmetric terms; lower triangle 0), g_harmonics (G,3,d_sh, with
 *   colour), g_opacities (G), summed over the views in ascending order.  Same inputs, values and workspace as the forward that filled
 *   them; a workspace may be read by another form's backward (colour + depth forward, colour-only backward).  slots: scratch of
 *   9 V max_keys floats without depth, 10 V max_keys with it, and that product must stay below 2^31. */
size_t mvsdet_splat_workspace_bytes(int V, int G, int H, int W, int max_keys);
int mvsdet_splat_cameras_f32(const float* extrinsics, int64_t ext_view_stride, const float* intrinsics, int64_t k_view_stride,
                             int64_t k_row_stride, const float* near, const float* far, int scale_invariant, float* cams, int V,
                             mvsdet_stream_t stream);
int mvsdet_splat_forward_f32(const float* means, const int64_t* means_strides /*HOST[2]*/, const float* covariances,
                             const int64_t* cov_strides /*HOST[3]*/, const float* harmonics, const int64_t* sh_strides /*HOST[3]*/,
                             const float* opacities, int64_t opacity_stride, const float* cams, const float* near, const float* far,
                             const float* background, float* image, float* depth, float* values, void* workspace,
                             size_t workspace_bytes, int V, int G, int d_sh, int use_sh, int with_colour, int with_depth, int mode, int H,
                             int W, int max_keys, mvsdet_stream_t stream);
int mvsdet_splat_backward_f32(const float* means, const int64_t* means_strides /*HOST[2]*/, const float* covariances,
                              const int64_t* cov_strides /*HOST[3]*/, const float* harmonics, const int64_t* sh_strides /*HOST[3]*/,
                              const float* opacities, int64_t opacity_stride, const float* cams, const float* near, const float* far,
                              const float* background, const float* g_image, const float* g_depth, const float* values,
                              void* workspace, size_t workspace_bytes, float* slots, float* g_means, float* g_covariances,
                              float* g_harmonics, float* g_opacities, int V, int G, int d_sh, int use_sh, int with_colour, int with_depth,
                              int mode, int H, int W, int max_keys, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian adapter (csrc/adapter.hip): the pixel Gaussians the rasteriser above renders -- GaussianAdapter.forward
 * (gs_src/model/encoder/common/gaussian_adapter.py:50-98) with the offset lines of mvsdet.py:576-578, for V source views of R = h w
 * feature pixels and S surfaces each.  Gaussian g = (v R + r) S + s, the reference's flattened order.  fp32, no atomics, no host
 * synchronisation; the same bits on every run.  DESIGN.md 4.16 has the formulas.
 * Limits: d_sh in {1, 4, 9, 16, 25}; V <= 65535; R = h w; R S (10 + 3 d_sh) < 2^31 (a view's rows); V R S 3 d_sh < 2^31.
 *
 * One row of `raw` has 9 + 3 d_sh floats: offset (2), scales (3), quaternion x y z w (4), harmonics (3, d_sh).  Row (v, r, s) starts
 *   at raw + v raw_view_stride + (r S + s) raw_row_stride (elements); its floats are adjacent.  g_raw is laid out by its own two strides.
 * mvsdet_adapter_cameras_f32 (one launch, one thread per view): cams (V, MVSDET_ADAPTER_CAM) = C_v = E_v[:3,:3] (9, row-major), the
 *   origin E_v[:3,3] (3), K_v^-1 by the adjugate (9), m_v = 0.1 sum_i (K_v[:2,:2]^-1 (1/w, 1/h))_i, 2 unused, then at float 24 the
 *   rotation blocks D_l of the harmonics, degree after degree (l = 0 .. 4: 1 + 9 + 25 + 49 + 81 floats, row-major; blocks above the
 *   degree of d_sh are 0), 3 unused.  sh_rot NULL: the blocks are built for the basis of csrc/sh_basis.h, sum_j (D c)_j Y_j(C d) =
 *   sum_j c_j Y_j(d), in float64 and rounded once.  sh_rot (V, sum_{l <= L} (2l+1)^2) contiguous: copied as given.
 * mvsdet_adapter_forward_f32 (one launch): depth (V,R) contiguous -> means (G,3), covariances (G,3,3: all nine), harmonics (G,3,d_sh),
 *   contiguous; scales (G,3) and rotations (G,4: the normalised quaternion) unless both NULL.
 * mvsdet_adapter_backward_f32 (one launch): g_means (G,3), g_covariances (G,3,3: any 3x3 gradient, symmetric or not), g_harmonics
 *   (G,3,d_sh), contiguous, each may be NULL (= zeros) -> g_raw (every float of every row written) and g_depth (V,R,S). */
#define MVSDET_ADAPTER_CAM 192
int mvsdet_adapter_cameras_f32(const float* extrinsics, int64_t ext_view_stride, const float* intrinsics, int64_t k_view_stride,
                               int64_t k_row_stride, const float* sh_rot /*may be NULL*/, float* cams, int V, int h, int w, int d_sh,
                               mvsdet_stream_t stream);
int mvsdet_adapter_forward_f32(const float* raw, int64_t raw_view_stride, int64_t raw_row_stride, const float* depth, const float* cams,
                               float* means, float* covariances, float* harmonics, float* scales /*may be NULL*/,
                               float* rotations /*may be NULL*/, int V, int h, int w, int S, int d_sh, float scale_min, float scale_max,
                               mvsdet_stream_t stream);
int mvsdet_adapter_backward_f32(const float* raw, int64_t raw_view_stride, int64_t raw_row_stride, const float* depth, const float* cams,
                                const float* g_means, const float* g_covariances, const float* g_harmonics, float* g_raw,
                                int64_t g_raw_view_stride, int64_t g_raw_row_stride, float* g_depth, int V, int h, int w, int S, int d_sh,
                                float scale_min, float scale_max, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian head (csrc/gshead.hip): `to_gaussians` = nn.Sequential(ReLU, Linear) of the novel-view branch (mvsdet.py:210-216) on the
 * rows extract_feat concatenates per source pixel (:561-569, process_rgb_raw :319-333), read in place -- no row matrix:
 *   raw[v][r][m] = bias[m] + sum_k weight[m][k] relu(x[k]),  r = y w + x over the h x w crop of the Hf x Wf map, and for source view
 *   ids[v]:  x[k] = feature[ids[v]][k][y][x] (k < C), x[C] = depth_coding[ids[v]][y][x], and with rgb (K = C + 4, else K = C + 1)
 *   x[C + 1 + c] = rgb_rows[v][r][c], or from images (N,3,Hi,Wi), Hi >= 4h - 1, Wi >= 4w - 1, the mean
 *   0.25 ((I[4y+1][4x+1] + I[4y+1][4x+2]) + (I[4y+2][4x+1] + I[4y+2][4x+2])) of image ids[v], channel c: what
 *   F.interpolate(scale_factor=0.25, mode='bilinear') gives.  Only ratio 4.  relu is torch's: NaN stays NaN.
 * Exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32), one output's products added in k order, the bias last.  No atomics, no
 * host synchronisation; the same bits on every run.  DESIGN.md 4.19.
 * Strides are HOST arrays of element strides, the w stride being 1: feature_strides[3] = n, c, h; depth_strides[2] = n, h of the
 * (N,h,w) map; image_strides[3] = n, c, h; all in [0, 2^40).  ids (V) int64 on the device, unique; an id outside [0, N) is never
 * used as an address: that view's raw is NaN and it gets no gradient.  weight (M,K), bias (M), raw and g (V,R,M), rgb_rows (V,R,3):
 * contiguous.  rgb_rows and images may both be NULL (no rgb) but not both be given.  Limits: V <= 65535, h w < 2^29.
 * mvsdet_gshead_forward_f32 (one launch) -> raw.   mvsdet_gshead_rgb_rows_f32 (one launch) -> rows (V,R,3): the image form alone.
 * mvsdet_gshead_backward_input_f32 (one launch): g_feature[ids[v]][k][y][x] = (x[k] > 0) sum_m weight[m][k] g[v][r][m] for the
 *   selected views' cropped pixels, g_depth_coding likewise; NOTHING else of the two buffers is written (the caller zeroes them).
 *   The rgb columns get no gradient.
 * mvsdet_gshead_backward_weight_f32 (two launches): g_weight (M,K) = sum_{v,r} g[v][r][m] relu(x[k]), g_bias (M) = sum_{v,r} g[v][r][m].
 *   The pixels (v, r) are cut into chunks of chunk_pixels (rounded up to a multiple of 32; 0 = the default, 256); chunk sums go to
 *   `partial` (mvsdet_gshead_partial_bytes; 0 for arguments the entry refuses) and are added in chunk order. */
int mvsdet_gshead_forward_f32(const float* feature, const int64_t* feature_strides /*HOST[3]*/, const float* depth_coding,
                              const int64_t* depth_strides /*HOST[2]*/, const float* rgb_rows /*may be NULL*/,
                              const float* images /*may be NULL*/, const int64_t* image_strides /*HOST[3], NULL without images*/,
                              const int64_t* ids, const float* weight, const float* bias, float* raw, int N, int V, int C, int K, int M,
                              int h, int w, int Hf, int Wf, int Hi, int Wi, mvsdet_stream_t stream);
int mvsdet_gshead_rgb_rows_f32(const float* images, const int64_t* image_strides /*HOST[3]*/, const int64_t* ids, float* rows, int N, int V,
                               int h, int w, int Hi, int Wi, mvsdet_stream_t stream);
int mvsdet_gshead_backward_input_f32(const float* feature, const int64_t* feature_strides /*HOST[3]*/, const float* depth_coding,
                                     const int64_t* depth_strides /*HOST[2]*/, const int64_t* ids, const float* weight, const float* g,
                                     float* g_feature, const int64_t* g_feature_strides /*HOST[3]*/, float* g_depth_coding,
                                     const int64_t* g_depth_strides /*HOST[2]*/, int N, int V, int C, int K, int M, int h, int w, int Hf,
                                     int Wf, mvsdet_stream_t stream);
size_t mvsdet_gshead_partial_bytes(int V, int R, int M, int K, int chunk_pixels);
int mvsdet_gshead_backward_weight_f32(const float* feature, const int64_t* feature_strides /*HOST[3]*/, const float* depth_coding,
                                      const int64_t* depth_strides /*HOST[2]*/, const float* rgb_rows /*may be NULL*/,
                                      const float* images /*may be NULL*/, const int64_t* image_strides /*HOST[3], NULL without images*/,
                                      const int64_t* ids, const float* g, float* g_weight, float* g_bias, float* partial,
                                      size_t partial_bytes, int chunk_pixels, int N, int V, int C, int K, int M, int h, int w, int Hf, int Wf,
                                      int Hi, int Wi, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The cost network's 3x3x3 convolutions on the bf16 matrix cores, fp32 operands cut into bf16 pieces ("bf16x3":
 * x*w ~ x_hi*w_hi + x_hi*w_mid + x_mid*w_hi, fp32 accumulation; csrc/costreg_bf16.hip).  Replaces the same layers of
 * mvs_models/mvsnet.py:76-82,104-108 as mvsdet_conv3d_k3_mfma_ws_f32 does, at 3/16 of the fp32 matrix-core time; results
 * differ from an fp32 convolution by ~2^-16 of the products' size (logits of the network: 2e-6 .. 4e-6, bar 1e-4).
 *
 * "SCL" (split channel-last) activations: xs[piece 2][n][c8 = ceil(C/8)][Dp][Hp][Wp][8] bf16, piece = hi | mid,
 * (dp,hp,wp) = (d,h,w) + 1 inside a zero border; Dp/Hp/Wp (the border plus the largest tile overhang of any kernel that
 * reads the form) and the size in bytes come from mvsdet_scl_bytes.
 * mvsdet_scl_pack_f32 cuts an (N,C,D,H,W) fp32 tensor (possibly row-pitched: mvsdet_plane_sweep_variance_tabled_pitched_f32; zero_border 1: clear the buffer first -- a buffer reused for the
 * same shape needs that once; 2: the packing kernel runs over the padded volume and writes the border's zeros itself -- for a
 * buffer fresh from an allocator on every call, no clearing pass).  weight_split (stride 1, for v_mfma_f32_16x16x32_bf16):
 * [Cout/64][c8][7 k-steps of 4 taps][4 groups of 16 outputs][2 pieces][64 lanes][8] bf16, lane = 16 * (tap of the k-step) + MFMA row m,
 * row m of group rg carrying output channel 32*(rg>>1) + 8*(m>>2) + 4*(rg&1) + (m&3) of the 64 (so that groups 2q, 2q+1 give a lane
 * eight consecutive channels = one SCL unit), tap 27 and channels >= Cin zero.  Stride 2 / transposed (v_mfma_f32_32x32x16_bf16): the same
 * bytes as [14 tap pairs][2 groups of 32 outputs][2 pieces][64 lanes][8], lane = 32 * (tap of the pair) + MFMA row m, row m carrying output
 * channel 8*((m>>4)*2 + ((m>>2)&1)) + (m&3) + 4*((m>>3)&1) of its group (mvsdet_amd.ops.split_conv_weight).
 * out (N,Cout,D,H,W) fp32 = [relu]([scale *] conv [+ shift] [+ residual]).  Stride 1, Cout % 64 == 0.
 * ------------------------------------------------------------------------------------------- */
size_t mvsdet_scl_bytes(int N, int C, int D, int H, int W, int* Dp /*HOST, may be NULL*/, int* Hp, int* Wp);
/* weight (Cout = 64*m, Cin, 3,3,3) fp32 -> weight_split (mvsdet_split_conv_weight_bytes) on the device: one small launch.
 * order 0 = the stride-1 layout above; 1 = for mvsdet_conv3d_k3_s2_bf16x3_io (tap pairs grouped by the parity class of the
 * input voxel); 2 = for the transposed convolution: `weight` is a ConvTranspose3d weight (Cin,Cout,3,3,3), pairs grouped by the
 * parity class of the output voxel. */
size_t mvsdet_split_conv_weight_bytes(int Cout, int Cin);
int mvsdet_split_conv_weight_ordered(const float* weight, void* weight_split, int Cout, int Cin, int order, mvsdet_stream_t stream);
/* up to 8 weight tensors in ONE launch (a network's layers: run per forward call, so in-place weight updates are always seen);
 * weights / weight_splits: HOST arrays of `count` device pointers; Cout / Cin / orders: HOST arrays */
int mvsdet_split_conv_weights_batched(const float* const* weights, void* const* weight_splits, const int* Cout, const int* Cin,
                                      const int* orders, int count, mvsdet_stream_t stream);
int mvsdet_scl_pack_f32(const float* x, const int64_t* x_strides /*HOST[4] = element strides of n, c, d, h; w stride 1; NULL = contiguous*/,
                        void* xs, int N, int C, int D, int H, int W, int zero_border, mvsdet_stream_t stream);
/* Workspace of the stride-1 / stride-2 convolution below (0: the grid is large enough unsplit).  Small volumes (the 3-D neck's
 * 20x20x8 and 10x10x4 levels: a handful of tiles): the input channels are split over blocks so that the grid fills the chip, raw
 * partial sums go to `workspace` and a second kernel adds them (ascending split order) before the affine, the residual and the
 * ReLU.  NULL or too small a workspace: unsplit, same results up to the order of the fp32 sums. */
size_t mvsdet_conv3d_k3_bf16x3_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W);
size_t mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W);

/* ---------------------------------------------------------------------------------------------
 * Layer-to-layer forms (round 4): a convolution can leave its result ALREADY CUT into bf16 pieces for the next one -- no fp32
 * round trip through a packing pass, the consumer feeds its LDS by DMA, and the producer issues one 16-byte store per piece
 * and 8 channels instead of eight 4-byte ones.  Chain of mvs_models/mvsnet.py:104-112:
 *   conv0 -(out_f32: skip of conv11, out_pscl)-> conv1 -(out_scl)-> conv2 -(out_f32: skip of conv9, out_pscl)-> conv3
 *   -(out_scl)-> conv4 -(out_scl)-> conv9 -(out_scl)-> conv11 -(out_f32)-> prob.
 * "PSCL" (parity-split SCL) of an (N,C,D,H,W) tensor: [piece 2][class 8][n][c8][cDp][cHp][cWp][8] bf16, class = 4*(d&1) +
 * 2*(h&1) + (w&1), voxel (d,h,w) at index (d/2+1, h/2+1, w/2+1) of its class, zero elsewhere: the eight stride-1 grids a
 * stride-2 convolution reads (mvsdet_pscl_bytes).  Output buffers' borders must be zero before the call (cleared once per
 * buffer: the kernels write interior voxels only); any of out_f32 / out_scl / out_pscl may be NULL.
 * ------------------------------------------------------------------------------------------- */
size_t mvsdet_pscl_bytes(int N, int C, int D, int H, int W, int* cDp /*HOST, may be NULL*/, int* cHp, int* cWp);
/* stride 1: input = xs (SCL) or x (the fp32 tensor itself, x_strides as for mvsdet_scl_pack_f32: the pieces are cut inside the
 * kernel while the previous channel group is multiplied -- no packing pass, no SCL copy; results identical bit for bit), exactly
 * one of them; weight_split of order 0; workspace (mvsdet_conv3d_k3_bf16x3_workspace_bytes) used only when out_f32 is the sole
 * output */
int mvsdet_conv3d_k3_bf16x3_io(const void* xs, const float* x, const int64_t* x_strides /*HOST[4], NULL = contiguous*/,
                               const void* weight_split, const float* scale, const float* shift, const float* residual,
                               float* out_f32, void* out_scl, void* out_pscl, void* workspace, size_t workspace_bytes, int N,
                               int Cin, int Cout, int D, int H, int W, int relu, mvsdet_stream_t stream);
/* stride 1 on ONE fp16 and TWO block-scaled FP6 (OCP MX e2m3) products per fp32-equivalent product instead of three bf16 ones
 * (csrc/costreg_mx.h; v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4): the layer that reads the fp32 variance volume in
 * place, mvs_models/mvsnet.py:76 (conv0).  x, x_strides, scale / shift / relu and the three outputs as for
 * mvsdet_conv3d_k3_bf16x3_io (no residual, no split over the input channels); weight_split_mx from mvsdet_split_conv_weight_mx
 * (mvsdet_split_conv_weight_mx_bytes).  Error per output: at most 2^-14 * sum over its products of (bmax |w| + wmax |x|) -- bmax the
 * largest finite |x| of the product's activation block (a tile's halo x 8 channels), wmax that of its weight block -- plus fp32
 * accumulation; about 2^-15 of the output's scale on data of uniform magnitude (bf16x3: 2^-16; whole-network logits 1-2e-5 from
 * float64, the bar is 1e-4), more on a small value beside a large one in its block.  A NaN or Inf input stays in its 3x3x3 receptive
 * field.  Inputs beyond fp16's range are cut on a block-uniform power of two (no cliff at 65504). */
size_t mvsdet_split_conv_weight_mx_bytes(int Cout, int Cin);   /* 0 unless Cout is a positive multiple of 64 */
int mvsdet_split_conv_weight_mx(const float* weight, void* weight_split_mx, int Cout, int Cin, mvsdet_stream_t stream);
int mvsdet_conv3d_k3_fp16mx_f32in(const float* x, const int64_t* x_strides /*HOST[4], NULL = contiguous*/, const void* weight_split_mx,
                                  const float* scale, const float* shift, float* out_f32, void* out_scl, void* out_pscl, int N, int Cin,
                                  int Cout, int D, int H, int W, int relu, mvsdet_stream_t stream);
/* 1 if the call above can address this view of x, else 0 (the call then fails with MVSDET_ERR_INVALID_ARG: use
 * mvsdet_conv3d_k3_bf16x3_io): the kernel reads a batch element's Cin channel volumes through one buffer descriptor with 32-bit
 * byte offsets, so Cin * sC * 4 plus the largest byte offset inside a channel volume must stay below 2^32 and the view's span
 * below the halo sentinel 0xfffffff0 -- e.g. Cin = 256 at 64 x 240 x 320 does not fit; with Cin % 8 != 0 (a pad channel is read)
 * the channel stride must also cover a channel volume's extent, which rules out channels interleaved with planes. */
int mvsdet_conv3d_k3_fp16mx_ok(int N, int Cin, int D, int H, int W, const int64_t* x_strides /*HOST[4], NULL = contiguous*/);
/* stride 1 in front of a training-mode BatchNorm (module.py:26-37 ConvBnReLU3D under model.train()): the raw fp32 output plus, from
 * the kernel's epilogue, per-channel partial sums of the outputs and of their squares -- stats[c * parts + i] = double2 of channel c
 * in block i of the grid, parts = mvsdet_conv3d_k3_bf16x3_stats_parts(N, D, H, W, x != NULL); stats_bytes >= Cout * parts * 16.
 * The sums are those of (value - pivot[c]) (pivot: Cout floats near the channels' means, e.g. the BatchNorm's running mean; NULL =
 * zeros): fp32 lane sums of raw values cancel when |mean| >> spread.  mvsdet_bn3d_relu_train_fwd_parts_f32 (same pivot) finishes
 * them: the BatchNorm reads the tensor once instead of twice. */
size_t mvsdet_conv3d_k3_bf16x3_stats_parts(int N, int D, int H, int W, int f32_input);
int mvsdet_conv3d_k3_bf16x3_stats(const void* xs, const float* x, const int64_t* x_strides /*HOST[4], NULL = contiguous*/,
                                  const void* weight_split, float* out_f32, void* stats, size_t stats_bytes, const float* pivot, int N,
                                  int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* ... and of the transposed layer (mvsnet.py:92-100): xs = SCL form of the coarse (N,Cin,D,H,W) input, out_f32 (N,Cout,2D,2H,2W) raw;
 * parts = mvsdet_convT3d_k3_s2_bf16x3_stats_parts(N, D, H, W), 0 where the shape has no statistics form (use the plain call then). */
size_t mvsdet_convT3d_k3_s2_bf16x3_stats_parts(int N, int D, int H, int W);
int mvsdet_convT3d_k3_s2_bf16x3_stats(const void* xs, const void* weight_split, float* out_f32, void* stats, size_t stats_bytes,
                                      const float* pivot, int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);
/* stride 2: Conv3d(kernel 3, stride 2, padding 1, no bias) [+ affine] [+ ReLU] (mvsnet.py:77,79), x (N,Cin,D,H,W) -> out
 * (N,Cout,(D-1)/2+1,(H-1)/2+1,(W-1)/2+1), Cout % 64 == 0; input = x (fp32 + x_strides) or x_pscl (the PSCL form of the input),
 * exactly one of them; weight_split of order 1; out_scl = SCL form of the result; workspace
 * (mvsdet_conv3d_k3_s2_bf16x3_workspace_bytes) used only when out_f32 is the sole output */
int mvsdet_conv3d_k3_s2_bf16x3_io(const float* x, const int64_t* x_strides /*HOST[4], NULL = contiguous*/, const void* x_pscl,
                                  const void* weight_split, const float* scale, const float* shift, float* out_f32,
                                  void* out_scl, void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int D, int H,
                                  int W, int relu, mvsdet_stream_t stream);
/* transposed: ConvTranspose3d(kernel 3, stride 2, padding 1, output_padding 1, no bias) [+ affine] [+ ReLU] [+ residual, added
 * last] (mvsnet.py:92-100,110-111): xs = SCL form of x (N,Cin,D,H,W); weight_split of order 2 from the (Cin,Cout,3,3,3) weight,
 * Cout % 64 == 0; out_f32 / residual (N,Cout,2D,2H,2W) fp32, 8-byte aligned; out_scl = SCL form of the result */
int mvsdet_convT3d_k3_s2_bf16x3_io(const void* xs, const void* weight_split, const float* scale, const float* shift,
                                   const float* residual, float* out_f32, void* out_scl, int N, int Cin, int Cout, int D, int H,
                                   int W, int relu, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement helper for bench.py: runs `fn`-independent HIP-event timing is done by the caller;
 * this only exposes a device-to-device float4 copy so the achievable HBM ceiling can be calibrated
 * on the same box (SURVEY.md section 8d "Roofline").
 * ------------------------------------------------------------------------------------------- */
int mvsdet_copy_f32(const float* src, float* dst, size_t n_floats, mvsdet_stream_t stream);

/* The plane sweep's store stream alone: the block -> address map of the fused variance kernel (mvsdet.py:467's volume,
 * (N,C,D,H,out_w_pitch) fp32; C % 32 == 0, W % 4 == 0), tile width 16 or 32, `planes_per_block` planes per block (0 = all),
 * 16-byte stores of the flavour option "sweep_store" selects (default: non-temporal) and nothing else.  bench.py times it to report what the output LAYOUT allows on the box at hand
 * (`frac_of_store_pattern_ceiling`); `var` is overwritten with arbitrary values. */
int mvsdet_store_pattern_probe_f32(float* var, int N, int C, int D, int H, int W, int out_w_pitch, int tile_w,
                                   int planes_per_block, mvsdet_stream_t stream);
/* The same for fp16 storage (BASELINE configs[4]): a lane's four pixels are 8 bytes, a wave-instruction writes 8 channel rows of
 * 64 bytes -- half a 128-byte line per row. */
int mvsdet_store_pattern_probe_f16(void* var, int N, int C, int D, int H, int W, int out_w_pitch, int tile_w,
                                   int planes_per_block, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The 3-D neck's GEMM-shaped layers (mmdet3d/models/necks/imvoxel_neck.py:166-180, 196-217) on the bf16 matrix cores with
 * three-term split operands, bias / ReLU / the 2x2x2 interleave in the epilogue (csrc/neck_gemm.hip).
 * wsplit = mvsdet_gemm_split_weight of the (M, K) fp32 row-major matrix with the eval-mode BatchNorm's scale folded in
 * (M % 128 == 0, K % 32 == 0): [M/32][K/16][2 pieces][64 lanes][8] bf16.
 *   mvsdet_conv3d_k1_s2_bf16x3:  out (N,Cout,D/2,H/2,W/2) = [relu](W (Cout,Cin) x[:, :, ::2, ::2, ::2] + bias), D, H, W even
 *   mvsdet_convT3d_k2_s2_bf16x3: out (N,Cout,2D,2H,2W)[.., 2d+p, 2h+q, 2w+r] = [relu](sum_c x[c][d][h][w] W[c][o][p][q][r] + bias[o]);
 *                                the matrix has the 8*Cout rows m = 8 o + 4 p + 2 q + r (ConvTranspose3d weight permuted (1,2,3,4,0))
 * ------------------------------------------------------------------------------------------- */
size_t mvsdet_gemm_split_weight_bytes(int M, int K);   /* 0 if (M, K) is not supported */
int mvsdet_gemm_split_weight(const float* wmat, void* wsplit, int M, int K, mvsdet_stream_t stream);
int mvsdet_conv3d_k1_s2_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, int N, int Cin, int Cout, int D,
                               int H, int W, int relu, mvsdet_stream_t stream);
int mvsdet_convT3d_k2_s2_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, int N, int Cin, int Cout, int D,
                                int H, int W, int relu, mvsdet_stream_t stream);
/* Their gradients under autograd (bf16x3, no atomics; split-K partial sums added in a fixed order: deterministic).
 *   mvsdet_conv3d_k1_s2_dx_bf16x3:  grad_x (N,Cin,D,H,W)[.., 2d, 2h, 2w] += sum_o W[o][c] grad_out (N,Cout,D/2,H/2,W/2)[.., d, h, w];
 *                                   only the even positions are written (accumulated into what grad_x holds); D, H, W even;
 *                                   wsplit = mvsdet_gemm_split_weight of the (Cin, Cout) matrix W^T (Cin % 128, Cout % 32)
 *   mvsdet_convT3d_k2_s2_dx_bf16x3: grad_x (N,Cin,D,H,W)[.., v] = sum_{o,p,q,r} W[c][o][p][q][r] grad_out (N,Cout,2D,2H,2W)[.., 2v + (p,q,r)];
 *                                   wsplit = mvsdet_gemm_split_weight of W.reshape(Cin, 8 Cout) (Cin % 128, 8 Cout % 32)
 *   mvsdet_neck_gemm_dw_bf16x3:     transposed = 0: dw (Cout, Cin) = sum_{n,v} grad_out (N,Cout,D,H,W)[o, v] x (N,Cin,2D,2H,2W)[c, 2v];
 *                                   transposed = 1: dw (Cin, Cout, 2,2,2) = sum_{n,v} x (N,Cin,D,H,W)[c, v] grad_out (N,Cout,2D,2H,2W)[o, 2v + pqr];
 *                                   (D, H, W) = the coarse grid; nsplit > 1 voxel chunks summed in `partial`
 *                                   (mvsdet_neck_gemm_dw_partial_bytes; 0 when nsplit <= 1: no buffer needed). */
int mvsdet_conv3d_k1_s2_dx_bf16x3(const float* grad_out, const void* wsplit, float* grad_x, int N, int Cin, int Cout, int D, int H,
                                  int W, mvsdet_stream_t stream);
int mvsdet_convT3d_k2_s2_dx_bf16x3(const float* grad_out, const void* wsplit, float* grad_x, int N, int Cin, int Cout, int D, int H,
                                   int W, mvsdet_stream_t stream);
size_t mvsdet_neck_gemm_dw_partial_bytes(int Cin, int Cout, int transposed, int nsplit);
int mvsdet_neck_gemm_dw_bf16x3(const float* x, const float* grad_out, float* dw, float* partial, size_t partial_bytes, int nsplit,
                               int transposed, int N, int Cin, int Cout, int D, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Level 0 of the 2-D feature pyramid in front of the sweep (mvsdet.py:374-376 `x = self.neck(x)[0]`) on the bf16 matrix cores with
 * three-term split operands (csrc/fpn.hip; gradients: csrc/fpn_bwd.hip, below).  fp32 in and out; no atomics (the same bits on every run).
 * The module is mmdet.models.necks.FPN as shipped: in_channels=[256,512,1024,2048], out_channels=256, num_outs=4, start_level=0, no
 * add_extra_convs, no norm, no activation, upsample_cfg=dict(mode='nearest').  mmdet is not part of this tree; this is the builder's
 * reading of it:
 *     L3 = lat3(c5);  L2 = lat2(c4) + up(L3);  L1 = lat1(c3) + up(L2);  L0 = lat0(c2) + up(L1);  out0 = conv3x3(L0) == FPN(inputs)[0]
 * lat_i = 1x1 convolution with bias, conv3x3 with padding 1 and bias, up = F.interpolate(size = the finer level's, mode='nearest'):
 * source index min((int)floorf(dst * ((float)in / (float)out)), in - 1) in float32, as ATen computes it (the integer form dst*in/out
 * differs, e.g. at 46 <- 14).  The 3x3 output convolutions of levels 1-3, which MVSDet drops, are not computed.
 *   mvsdet_fpn_lateral_bf16x3: out (N,Cout,H,W) = W (Cout,Cin) x (N,Cin,H,W) + bias [+ top (N,Cout,Ht,Wt) at the nearest source index];
 *       top NULL = no addition (Ht, Wt ignored), else 1 <= Ht <= H, 1 <= Wt <= W.  wsplit = mvsdet_gemm_split_weight of the (Cout, Cin)
 *       matrix; Cin % 32 == 0, Cout % 128 == 0, any H, W >= 1, N H W < 2^31.  Contiguous tensors.
 *   mvsdet_fpn_conv3x3_bf16x3: conv3x3(x (N,Cin,H,W)) + bias, zero padding 1, written as fp32 (N,Cout,H,W) to `out` and / or as packed
 *       maps (mvsdet_packed_bytes(N,Cout,H,W), what mvsdet_pack_features_f32 makes of `out`) to `packed`: each where its pointer is not
 *       NULL, at least one.  wsplit = mvsdet_gemm_split_weight of the (Cout, 9 Cin) tap-major matrix w.permute(0,2,3,1).reshape(Cout, 9 Cin)
 *       (k = Cin (3 dy + dx) + c); Cin % 32 == 0, Cout % 128 == 0, N <= 65535.  packed 16-byte aligned.
 * Values (both entries, and the input gradients that run on them; tests/test_gpu_backbone_edges.py).  The range is fp32's: x is cut
 * into two bf16 pieces inside the kernel, so x 2^k gives out 2^k bit for bit while nothing over- or underflows (bias and top zero), and
 * every |x| <= 0x7f7f7f80, the largest value two pieces hold, keeps a finite hi piece.
 *     Non-finite x: an infinity (hi = inf, mid = inf - inf) and a finite |x| >= 0x7f7f8000 (it rounds to an infinite hi, mid = -inf) yield
 *     NaN, not inf, in the receptive field of that element.
 *     A NaN (or the NaN such a value yields) reaches exactly the receptive field of its element: every output channel -- a zero weight
 *     does not stop it, 0 * NaN = NaN -- at the pixels that read it, in its own view; every other output element keeps its bits, in
 *     `out` and in `packed`.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_fpn_lateral_bf16x3(const float* x, const void* wsplit, const float* bias, const float* top, float* out, int N, int Cin,
                              int Cout, int H, int W, int Ht, int Wt, mvsdet_stream_t stream);
int mvsdet_fpn_conv3x3_bf16x3(const float* x, const void* wsplit, const float* bias, float* out, float* packed, int N, int Cin, int Cout,
                              int H, int W, mvsdet_stream_t stream);
/* Its gradients (csrc/fpn_bwd.hip; no atomics, every sum in a fixed order: the same bits on every run).  The two input gradients are
 * the forward entries above: gL0 = mvsdet_fpn_conv3x3_bf16x3 on the flipped, transposed weight w3'[c,o,dy,dx] = w3[o,c,2-dy,2-dx] with a
 * zero bias, dx_i = mvsdet_fpn_lateral_bf16x3 on the split of W_i^T (C_i, Cout) with a zero bias and no top (so C_i % 128 == 0).
 *   mvsdet_fpn_dw_bf16x3: the weight gradient of a 1x1 (taps = 1) or 3x3 padding-1 (taps = 9) convolution, bf16x3 with the PIXELS as the
 *       reduction: dw (Cout,C,kh,kw)[o,c,dy,dx] = sum_{n,y,x} gy (N,Cout,H,W)[n,o,y,x] x (N,C,H,W)[n,c,y+dy-1,x+dx-1] (zero outside; taps = 1:
 *       dy = dx = 1 only).  The kernel's channel rule: C % 32 == 0 (a block's 32 input channels), Cout % 128 == 0; N <= 65535,
 *       N H W < 2^31; any H, W >= 1; 4-byte aligned contiguous tensors.  K is split over mvsdet_fpn_dw_splits(...) blocks, each writing
 *       its fp32 partial to `workspace` (at least mvsdet_fpn_dw_workspace_bytes(...) bytes, 4-byte aligned); the same entry then adds the
 *       splits in ascending order into dw.  Both queries are host only and return 0 for a shape the kernel refuses.
 *       Values: fp32's range (gy 2^k against x 2^-k keeps dw's bits).  A non-finite gy[n,o,..] (NaN, an infinity, a finite value of
 *       magnitude >= 0x7f7f8000) stays in ROW o of dw, one in x[n,c,..] in COLUMN c: every other row (column) keeps its bits.  Inside
 *       that row (column) the taps that pair the element with an element of the other map are NaN; further taps may be NaN as well (the
 *       padding and the ragged edge of a tile are zeros that are multiplied: 0 * NaN), which nothing promises either way.
 *   mvsdet_fpn_top_down_grad_f32: the adjoint of the top-down nearest gather: gt (N,C,Ht,Wt)[.., yt, xt] = the sum of g (N,C,H,W) over the
 *       pixels whose source index (the float32 one above) is (yt, xt), rows ascending, then columns ascending; 1 <= Ht <= H, 1 <= Wt <= W.
 *   mvsdet_fpn_bias_grad_f32: db (C) = the sum of g (N,C,H,W) over views and pixels. */
int mvsdet_fpn_dw_splits(int taps, int N, int C, int Cout, int H, int W);
size_t mvsdet_fpn_dw_workspace_bytes(int taps, int N, int C, int Cout, int H, int W);
int mvsdet_fpn_dw_bf16x3(const float* gy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int taps, int N, int C, int Cout,
                         int H, int W, mvsdet_stream_t stream);
int mvsdet_fpn_top_down_grad_f32(const float* g, float* gt, int N, int C, int H, int W, int Ht, int Wt, mvsdet_stream_t stream);
int mvsdet_fpn_bias_grad_f32(const float* g, float* db, int N, int C, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The bottleneck layers of the 2-D backbone (ResNet-50, style='pytorch', norm_eval=True, frozen BatchNorm) on the bf16 matrix cores
 * with three-term split operands (csrc/resnet.hip).  fp32 NCHW in and out; no atomics (the same bits on every run); 64-bit element
 * offsets.  mmdet is not part of this tree; this is the builder's reading of ResNet v1.5 (`torchvision://resnet50`):
 *     bottleneck(x; planes p, stride s): a = relu(bn1(conv1x1(x)));  b = relu(bn2(conv3x3(a, stride s, pad 1)));  c = bn3(conv1x1(b));
 *         id = bn_d(conv1x1(x, stride s)) where the block has a downsample branch, else x;  out = relu(c + id)
 *     layer1..4 = (3, 4, 6, 3) blocks of planes (64, 128, 256, 512), strides (1, 2, 2, 2), the first block of each with the branch;
 *     bn(y) = y * scale + shift, scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale;  no convolution has a bias.
 * A strided layer's output is ((H - 1) / s + 1) x ((W - 1) / s + 1).  `scale` is folded into the weight rows on the host BEFORE the
 * split; `shift` is the kernels' per-channel addend.  The matrix handed in has ceil(Cout / 128) * 128 rows, those from Cout on zero
 * (mvsdet_gemm_split_weight wants M % 128 == 0); nothing is stored for them.  The epilogue order is fixed: (acc + shift) + residual, then
 * ReLU as `v < 0 ? 0 : v`, so a NaN stays a NaN (torch.relu's rule).
 *   mvsdet_resnet_conv1x1_bf16x3: out (N,Cout,Ho,Wo) = [relu]( (W' x[.., s y, s x] + shift) [+ residual (N,Cout,Ho,Wo)] ); residual may
 *       be NULL.  wsplit = the split of the (ceil128(Cout), Cin) matrix.  The GEMM's columns run over all views' output pixels.
 *   mvsdet_resnet_conv3x3_bf16x3: out (N,Cout,Ho,Wo) = [relu]( conv3x3(x, stride s, zero padding 1) + shift ).  wsplit = the split of the
 *       (ceil128(Cout), 9 Cin) tap-major matrix w'.permute(0,2,3,1).reshape(Cout, 9 Cin), zero rows appended (k = Cin (3 dy + dx) + c).
 *       N <= 65535.
 * Both: stride 1 or 2; Cin % 32 == 0, Cout % 32 == 0; any H, W >= 1 with H W < 2^31; N Ho Wo < 2^31; wsplit 16-byte aligned, contiguous
 * 4-byte aligned tensors; relu 0 or 1.  Everything else is refused on the host before any launch.
 * Values (tests/test_gpu_backbone_edges.py).  The range is fp32's: x is cut into two bf16 pieces inside the kernel, so x 2^k gives
 * out 2^k bit for bit while nothing over- or underflows (shift zero, no residual), and every |x| <= 0x7f7f7f80, the largest value two
 * pieces hold, keeps a finite hi piece.
 *     Non-finite x: an infinity (hi = inf, mid = inf - inf) and a finite |x| >= 0x7f7f8000 (it rounds to an infinite hi, mid = -inf) yield
 *     NaN, not inf, in the receptive field of that element.
 *     A NaN (or the NaN such a value yields) reaches exactly the receptive field of its element: every output channel -- a zero weight
 *     does not stop it -- at the output pixels that read it (the strided 1x1 reads even pixels only), in its own view, through shift,
 *     residual and ReLU; every other output element keeps its bits.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_resnet_conv1x1_bf16x3(const float* x, const void* wsplit, const float* shift, const float* residual, float* out, int N, int Cin,
                                 int Cout, int H, int W, int stride, int relu, mvsdet_stream_t stream);
int mvsdet_resnet_conv3x3_bf16x3(const float* x, const void* wsplit, const float* shift, float* out, int N, int Cin, int Cout, int H, int W,
                                 int stride, int relu, mvsdet_stream_t stream);
/* Their gradients (csrc/resnet_bwd.hip; no atomics, every sum in a fixed order: the same bits on every run).  One bottleneck, g = dL/dout:
 *     gz = gate(g, out);  dW3 = scale3 (.) (gz b^T);  gb = gate(W3'^T gz, b);  dW2 = scale2 (.) dw3x3_s(gb, a);
 *     ga = gate(convT3x3_s(gb; W2'), a);  dW1 = scale1 (.) (ga x^T);  dx = (W1'^T ga) + (gz | spread_s(Wd'^T gz));
 *     dWd = scaled (.) (gz x[.., s y, s x]^T);   spread_s puts (yo, xo) at (s yo, s xo), zero elsewhere
 * gate(v, y) = y <= 0 ? 0 : v on the SAVED OUTPUT y of the ReLU: ATen's threshold_backward, the gradient rule of torch.relu.  The gradient
 * becomes +0.0 where y is 0.0, -0.0 or negative (whatever v holds, a NaN included) and passes where y is positive, +inf or NaN.  The rows'
 * `scale (.)` is the caller's; the stride-1 weight gradients are mvsdet_fpn_dw_bf16x3.  In every entry C = the layer's INPUT channels (the
 * rows of the GEMM, any multiple of 32: the matrix handed in has ceil(C / 128) * 128 rows, those from C on zero) and Cout = its output
 * channels (the reduction, a multiple of 32); `gate` = the gate map at the output's shape, NULL = no gate.
 *   mvsdet_resnet_relu_gate_f32: out[e] = gate(g[e], y[e]) for `total` elements.
 *   mvsdet_resnet_conv1x1_dx_bf16x3: out (N,C,H,W) = gate( (W'^T g (N,Cout,H,W)) [+ residual], gate ), the additions in that order.  wsplit =
 *       the split of the (ceil128(C), Cout) matrix W'^T.  residual NULL = none; spread = 1: residual (N,C,H,W); spread = 2: residual
 *       (N,C,(H-1)/2+1,(W-1)/2+1) added at (y / 2, x / 2) where y and x are both even, nothing added elsewhere.  N H W < 2^31.
 *   mvsdet_resnet_conv3x3_dx_bf16x3: out (N,C,H,W) = gate( convT3x3_s(g (N,Cout,Ho,Wo); W'), gate ), the input gradient of the padding-1 3x3 of
 *       stride s at an input of H x W (Ho = (H-1)/s+1).  s = 1: wsplit = the split of the (ceil128(C), 9 Cout) tap-major matrix of the
 *       flipped, transposed weight w'[c,o,dy,dx] = W'[o,c,2-dy,2-dx]; one launch.  s = 2: the inserted zeros are never multiplied: the
 *       pixels fall into four parity classes (py, px) = (y & 1, x & 1) of (1+py)(1+px) taps (dy = 1 for an even y; dy = 0, 2 for an odd
 *       one, reading output rows (y+1)/2 and (y-1)/2), one GEMM launch each; wsplit = the four classes' splits behind one another in the
 *       order (0,0), (0,1), (1,0), (1,1), class (py, px) the (ceil128(C), taps Cout) matrix with column (tap index) Cout + o holding
 *       W'[o,c,dy,dx], the class's taps ordered dy ascending, then dx ascending.  N <= 65535, N H W < 2^31.
 *   mvsdet_resnet_dw_s2_bf16x3: the weight gradient of a stride-2 1x1 (taps = 1) or padding-1 3x3 (taps = 9) convolution, bf16x3 with the
 *       OUTPUT pixels as the reduction: dw (Cout,C,kh,kw)[o,c,dy,dx] = sum_{n,yo,xo} gy (N,Cout,Ho,Wo)[n,o,yo,xo] x (N,C,H,W)[n,c,2yo+dy-1,
 *       2xo+dx-1] (zero outside; taps = 1: dy = dx = 1 only).  Only the real multiply-adds.  C % 32 == 0, Cout % 128 == 0, N <= 65535,
 *       H W < 2^31, N Ho Wo < 2^31.  K is split over mvsdet_resnet_dw_s2_splits(...) blocks, each writing its fp32 partial to `workspace` (at
 *       least mvsdet_resnet_dw_s2_workspace_bytes(...) bytes; a shorter one: MVSDET_ERR_WORKSPACE); the same entry then adds the splits in
 *       ascending order into dw.  Both queries are host only and return 0 for a shape the kernel refuses.
 * All: wsplit 16-byte aligned, contiguous 4-byte aligned tensors; everything else is refused on the host before any launch.
 * Values (tests/test_gpu_backbone_edges.py): fp32's range, as the forward entries.
 *     The input gradients: a non-finite g[n,o,yo,xo] (NaN, an infinity, a finite magnitude >= 0x7f7f8000: all three come out as NaN)
 *     reaches exactly the input pixels that output pixel was computed from -- 1x1: the pixel itself; 3x3: (s yo + dy - 1, s xo + dx - 1)
 *     inside the map -- in every channel of view n; every other element keeps its bits.  Under a gate a dropped position is +0.0
 *     whatever reached it, so the NaNs are the field's positions whose gate passes.
 *     The stride-2 weight gradient: a non-finite gy[n,o,..] stays in ROW o of dw, one in x[n,c,..] in COLUMN c (an x the convolution never
 *     reads, an odd pixel under taps = 1, changes nothing); the taps that pair the element with an element of the other map are NaN,
 *     further taps of that row (column) may be (0 * NaN at the padding and the ragged edge), which nothing promises either way. */
int mvsdet_resnet_relu_gate_f32(const float* g, const float* y, float* out, long long total, mvsdet_stream_t stream);
int mvsdet_resnet_conv1x1_dx_bf16x3(const float* g, const void* wsplit, const float* residual, const float* gate, float* out, int N, int C,
                                    int Cout, int H, int W, int spread, mvsdet_stream_t stream);
int mvsdet_resnet_conv3x3_dx_bf16x3(const float* g, const void* wsplit, const float* gate, float* out, int N, int C, int Cout, int H, int W,
                                    int stride, mvsdet_stream_t stream);
int mvsdet_resnet_dw_s2_splits(int taps, int N, int C, int Cout, int H, int W);
size_t mvsdet_resnet_dw_s2_workspace_bytes(int taps, int N, int C, int Cout, int H, int W);
int mvsdet_resnet_dw_s2_bf16x3(const float* gy, const float* x, float* dw, void* workspace, size_t workspace_bytes, int taps, int N, int C,
                               int Cout, int H, int W, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Detection post-processing of the ScanNet head (NerfDetHead.predict_by_feat / _nms / aligned_3d_nms, nerfdet_head.py:301-420,
 * 564-628) on the caller's stream, no host synchronisation (csrc/detect.hip).  fp32; labels int64.
 *
 * mvsdet_detect_head_f32: B scenes, L levels (HOST arrays of L device pointers: center (B,1,X,Y,Z), bbox (B,6,X,Y,Z), cls
 *   (B,C,X,Y,Z), contiguous; level_dims HOST int[3 L]); valid (B,1,VX,VY,VZ) = the stacked view counts as float; level_geom
 *   (B,L,6) DEVICE float = per scene and level the voxel size and get_points' new_origin.  Per level k = nms_pre if
 *   X*Y*Z > nms_pre > 0, else X*Y*Z; ncap = the sum of k over the levels, points = the sum of X*Y*Z.  Outputs padded to Nmax >=
 *   min(ncap, MVSDET_DETECT_MAX_CANDIDATES): out_boxes (B,Nmax,6) (cx, cy, cz, dx, dy, dz), out_scores (B,Nmax), out_labels
 *   (B,Nmax), out_count (B) int32; rows past a scene's count are zero.  A scene with more than MVSDET_DETECT_MAX_CANDIDATES
 *   boxes above score_thr gets out_count = -(that number) and no boxes (known on the device only).
 *   Candidate order: score descending, ties by level, then voxel index (the reference's argsort leaves ties unordered).
 * mvsdet_aligned_3d_nms_f32: boxes (n,6) (x1,y1,z1,x2,y2,z2), scores (n), classes (n) int64 -> out_index (n) int64 = the kept
 *   indices in pick order, out_count (1) int32; n <= MVSDET_DETECT_MAX_CANDIDATES (else MVSDET_ERR_INVALID_ARG).
 * mvsdet_detect_workspace_bytes(B, points, ncap): the workspace of either call (standalone NMS: B = 1, points = 0, ncap = n);
 *   each region rounded up to 256 bytes, caps = min(ncap, limit):
 *   B*4*4 + B*4 + 2 * B*points*4 + B*ncap*(24+4+8) (three regions) + B*caps*(24+4+8+4) (four) + B*caps*ceil(caps/64)*8.
 * ------------------------------------------------------------------------------------------- */
#define MVSDET_DETECT_MAX_CANDIDATES 16384 /* boxes of one scene above score_thr: one sort in 128 KiB of LDS */
#define MVSDET_DETECT_MAX_LEVELS 4
size_t mvsdet_detect_workspace_bytes(int B, int points, int ncap);
int mvsdet_detect_head_f32(const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                           const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ,
                           int nms_pre, float score_thr, float iou_thr, float* out_boxes, float* out_scores, int64_t* out_labels,
                           int* out_count, int nmax, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);
int mvsdet_aligned_3d_nms_f32(const float* boxes, const float* scores, const int64_t* classes, int n, float thresh,
                              int64_t* out_index, int* out_count, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Detection post-processing of the ARKit head (ImVoxelHead_ARKit.predict_by_feat / _single_scene_multiclass_nms / mmcv's nms3d,
 * nerfdet_head.py:902-1056, 1190-1243) on the caller's stream, no host synchronisation (csrc/detect.hip).  fp32; labels int64.
 *
 * mvsdet_detect_head_rotated_f32: the arguments of mvsdet_detect_head_f32, with bbox maps of 7 channels (six distances and the
 *   angle) and n_classes <= 256, B * n_classes <= 65535.  Every top-k point is decoded into a (x, y, z, dx, dy, dz, heading) box;
 *   each of its classes with a score > score_thr puts it into the scene's segment of that class; nms3d runs per segment (order: the
 *   class score descending, ties by level, then voxel index).  Outputs padded to Nmax >= n_classes * min(ncap,
 *   MVSDET_DETECT_MAX_CANDIDATES): out_boxes (B,Nmax,7), out_scores (B,Nmax), out_labels (B,Nmax), out_count (B) int32, class-major
 *   (classes ascending, each in pick order); rows past a scene's count are zero.  A scene with more than
 *   MVSDET_DETECT_MAX_CANDIDATES boxes above score_thr in one class gets out_count = -(the largest such number) and no boxes.
 * mvsdet_nms3d_f32: mmcv's nms3d of one class: boxes (n,7), scores (n) -> out_index (n) int64 = the kept indices in pick order,
 *   out_count (1) int32; suppression where iou_bev(kept, later) > thresh; n <= MVSDET_DETECT_MAX_CANDIDATES.
 * mvsdet_bev_iou_rotated_f32: out (n,m) = iou_bev(a[i], b[j]) of boxes (n,7) and (m,7): the device function of both calls above.
 * mvsdet_detect_rotated_workspace_bytes(B, points, ncap, n_classes): the workspace of either NMS call (standalone: B = 1,
 *   points = 0, ncap = n, n_classes = 1); each region rounded up to 256 bytes, S = B*n_classes, caps = min(ncap, limit):
 *   3 * S*4 + B*points*4 + B*ncap*28 + S*ncap*4 + S*caps*(4+28+4+4+56+4) (six regions) + S*caps*ceil(caps/64)*8.
 * ------------------------------------------------------------------------------------------- */
size_t mvsdet_detect_rotated_workspace_bytes(int B, int points, int ncap, int n_classes);
int mvsdet_detect_head_rotated_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                   const int* level_dims, const float* valid, const float* level_geom, int B, int L, int n_classes,
                                   int VX, int VY, int VZ, int nms_pre, float score_thr, float iou_thr, float* out_boxes,
                                   float* out_scores, int64_t* out_labels, int* out_count, int nmax, void* workspace,
                                   size_t workspace_bytes, mvsdet_stream_t stream);
int mvsdet_nms3d_f32(const float* boxes, const float* scores, int n, float thresh, int64_t* out_index, int* out_count,
                     void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);
int mvsdet_bev_iou_rotated_f32(const float* a, int n, const float* b, int m, float* out, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training of the ScanNet head (csrc/assign.hip): target assignment (NerfDetHead._get_targets, nerfdet_head.py:473-562) and the
 * three losses of _loss_by_feat_single (:206-257) on the caller's stream, no host synchronisation, no float atomics (the same bits
 * from run to run).  fp32; labels int64.  Levels, level_dims, level_geom and valid as in mvsdet_detect_head_f32; P = a scene's
 * points, the levels concatenated in order, a level's voxels x-major.
 *
 * mvsdet_head_targets_f32: gt_boxes (B,G,6) = (gravity centre, size), gt_volumes (B,G), gt_labels (B,G) int64, padded to the
 *   batch's largest G <= MVSDET_ASSIGN_MAX_BOXES; gt_counts (B) int32 DEVICE = boxes of every scene.  Outputs: out_labels (B,P)
 *   int64 (-1: no box), out_box_index (B,P) int32 (-1), out_center_targets (B,P), out_bbox_targets (B,P,6) (zero where no box).
 *   A point takes the box of least volume among those it lies inside, on the box's best level, with centerness above the box's
 *   (pts_center_threshold + 1)-th largest (strictly); equal volumes: the lowest box index.  A scene without boxes: every label -1.
 *   Workspace: B * G * (MVSDET_DETECT_MAX_LEVELS + 2) * 4 bytes (0 for G = 0: none needed).
 * mvsdet_head_loss_f32: the unnormalised sums of every scene: out_sums (B,4) = (sum over positive points of the centerness BCE,
 *   sum of centerness target * (1 - IoU), sum over valid points and classes of mmcv's sigmoid focal loss, sum of the centerness
 *   targets), out_counts (B,2) int32 = (positive points, valid points); positive = label >= 0 and valid.
 *   Workspace: B * ceil(P / 256) * 6 * 4 bytes.
 * mvsdet_head_loss_backward_f32: coef (B,3) DEVICE = what a unit of a scene's centerness / box / classification sum is worth
 *   (incoming gradient over the normaliser); d_center, d_bbox, d_cls: HOST arrays of L device pointers, written densely in the maps'
 *   layouts (zero where a point takes no part).
 * ------------------------------------------------------------------------------------------- */
#define MVSDET_ASSIGN_MAX_BOXES 1024 /* ground-truth boxes of one scene: staged in 36 KiB of LDS (48 KiB with headings) */
size_t mvsdet_head_targets_workspace_bytes(int B, int G);
int mvsdet_head_targets_f32(const int* level_dims, const float* level_geom, int B, int L, const float* gt_boxes,
                            const float* gt_volumes, const int64_t* gt_labels, const int* gt_counts, int G, int pts_assign_threshold,
                            int pts_center_threshold, int64_t* out_labels, int* out_box_index, float* out_center_targets,
                            float* out_bbox_targets, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);
size_t mvsdet_head_loss_workspace_bytes(int B, int points);
int mvsdet_head_loss_f32(const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                         const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ,
                         const int64_t* labels, const float* center_targets, const float* bbox_targets, float gamma, float alpha,
                         float* out_sums, int* out_counts, void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);
int mvsdet_head_loss_backward_f32(const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                                  const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ,
                                  const int64_t* labels, const float* center_targets, const float* bbox_targets, float gamma,
                                  float alpha, const float* coef, float* const* d_center, float* const* d_bbox, float* const* d_cls,
                                  mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training of the ARKit head (csrc/assign.hip, the same kernels instantiated for 7-value boxes): ImVoxelHead_ARKit._get_targets
 * (nerfdet_head.py:1107-1185) and _loss_by_feat_single (:779-846) with RotatedIoU3DLoss.  Everything as in the three entries above
 * except:
 *
 * mvsdet_head_targets_rotated_f32: gt_boxes (B,G,7) = (gravity centre, size, yaw); gt_rot (B,G,2) = (cos(yaw), sin(yaw)) as the
 *   caller computed them (no transcendental is evaluated on the way to a label).  Face distances are taken in the box's own frame
 *   (:1058-1084).  The top-k takes min(pts_center_threshold + 1, P) values.  out_bbox_targets (B,P,7) = the chosen ground-truth row
 *   itself (zero where no box); out_center_targets is -1 where no box is assigned.  Workspace: mvsdet_head_targets_workspace_bytes.
 * mvsdet_head_loss_rotated_f32 / mvsdet_head_loss_rotated_backward_f32: bbox maps of 7 channels (six distances, heading),
 *   bbox_targets (B,P,7); the box term is centerness target * (1 - IoU3D) of the decoded rotated box (:1029-1055) and its target,
 *   IoU3D = A_bev * z overlap / (V_pred + V_gt - A_bev * z overlap), A_bev the exact area of the intersection of the two rotated
 *   rectangles.  Relative headings within 1e-6 rad of a multiple of pi/2 count as that multiple; an edge shared by both rectangles
 *   counts once; every value and gradient is finite, a target of zero size gives IoU 0.  The targets receive no gradient.
 *   Workspace: mvsdet_head_loss_workspace_bytes.
 * ------------------------------------------------------------------------------------------- */
int mvsdet_head_targets_rotated_f32(const int* level_dims, const float* level_geom, int B, int L, const float* gt_boxes,
                                    const float* gt_rot, const float* gt_volumes, const int64_t* gt_labels, const int* gt_counts, int G,
                                    int pts_assign_threshold, int pts_center_threshold, int64_t* out_labels, int* out_box_index,
                                    float* out_center_targets, float* out_bbox_targets, void* workspace, size_t workspace_bytes,
                                    mvsdet_stream_t stream);
int mvsdet_head_loss_rotated_f32(const float* const* center, const float* const* bbox, const float* const* cls, const int* level_dims,
                                 const float* valid, const float* level_geom, int B, int L, int n_classes, int VX, int VY, int VZ,
                                 const int64_t* labels, const float* center_targets, const float* bbox_targets, float gamma,
                                 float alpha, float* out_sums, int* out_counts, void* workspace, size_t workspace_bytes,
                                 mvsdet_stream_t stream);
int mvsdet_head_loss_rotated_backward_f32(const float* const* center, const float* const* bbox, const float* const* cls,
                                          const int* level_dims, const float* valid, const float* level_geom, int B, int L,
                                          int n_classes, int VX, int VY, int VZ, const int64_t* labels, const float* center_targets,
                                          const float* bbox_targets, float gamma, float alpha, const float* coef,
                                          float* const* d_center, float* const* d_bbox, float* const* d_cls, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Indoor detection metrics (mmdet3d's indoor_eval: per-class AP and recall at IoU thresholds; csrc/evalmap.hip) on the caller's
 * stream, no host synchronisation, no device allocation.  Boxes are the box classes' own rows (x, y, BOTTOM z, dx, dy, dz, yaw),
 * fp32; labels int64 in [0, n_labels).  The IoU is BaseInstance3DBoxes.overlaps as a mathematical function in float32 (height
 * overlap x exact area of the intersection of the two footprints, extents clamped to >= 1e-4, over clamp(v1 + v2 - overlap,
 * 1e-8)); mmcv's box_iou_rotated rounding is not reproduced.  This is NOT iou_bev of mvsdet_bev_iou_rotated_f32.
 *
 * State: one DEVICE buffer of mvsdet_eval_state_bytes(n_labels, capacity, gt_capacity) bytes (0: bad sizes), 8-byte aligned,
 *   cleared by mvsdet_eval_reset; capacity = detections, gt_capacity = ground-truth boxes the evaluator can take in all.  The same
 *   three sizes go to every call on a state.
 * mvsdet_eval_match_f32: a batch of B scenes: pred (B,Nmax,7), scores (B,Nmax), labels (B,Nmax), counts (B) int32; gt (B,G,7),
 *   gt_labels (B,G), gt_counts (B) int32; scene0 = serial number of the batch's first scene, not below the serials already fed.
 *   Appends one record per detection (score, label, scene, row, global slot of the best-overlapping ground-truth box of its label in
 *   its scene -- the FIRST of equal IoUs -- and that IoU, -inf without such a box) and adds the ground-truth counts per label.  A
 *   batch that would run over a capacity, a count that is negative or above Nmax / G, and a serial below the state's set a flag of
 *   MVSDET_EVAL_FLAG_* in the state and write nothing else; a label outside [0, n_labels) sets MVSDET_EVAL_FLAG_BAD_LABEL.
 * mvsdet_eval_compute: n_bound = a HOST upper bound of the records fed (<= capacity; fewer records than fed sets
 *   MVSDET_EVAL_FLAG_BOUND); thresholds: HOST float[n_thr], compared in float32 (iou_max > t).  Visiting order: label, score
 *   descending (NaN last, -0 = +0), scene serial, row.  Outputs: out_ap (n_thr,n_labels) float32 = the area AP of
 *   average_precision; out_recall (n_thr,n_labels) float64 = the final recall; out_npos, out_ndet (n_labels) int32; out_first
 *   (n_labels) int64 = scene << 32 | ground truth << 31 | row where the label was first seen (-1: never), the order of the
 *   reference's dicts; out_tp (n_thr,n_bound) uint8 = true-positive flag of every record in visiting order; out_order (n_bound)
 *   int32 = the records' feeding index in visiting order; out_info (4) int32 = records, ground-truth slots, flags, next serial.  A
 *   label that is predicted and has no ground truth gives NaN AP and recall, as the reference does; a label without predictions 0.
 *   The state is left as it is: more batches may follow.  Workspace: mvsdet_eval_workspace_bytes(n_labels, n_bound, gt_capacity,
 *   n_thr) (0: bad sizes), 8-byte aligned.
 * mvsdet_eval_iou_f32: out (n,m) = the evaluator's IoU of boxes a (n,7) and b (m,7).
 * ------------------------------------------------------------------------------------------- */
#define MVSDET_EVAL_MAX_RECORDS (1 << 20) /* 20 bits of a sort key */
#define MVSDET_EVAL_MAX_LABELS 4095       /* 12 bits of a sort key, all ones kept for padding */
#define MVSDET_EVAL_MAX_THRESHOLDS 8
#define MVSDET_EVAL_FLAG_RECORDS_FULL 1
#define MVSDET_EVAL_FLAG_SLOTS_FULL 2
#define MVSDET_EVAL_FLAG_BAD_COUNT 4
#define MVSDET_EVAL_FLAG_SERIAL 8
#define MVSDET_EVAL_FLAG_BAD_LABEL 16
#define MVSDET_EVAL_FLAG_BOUND 32
size_t mvsdet_eval_state_bytes(int n_labels, int capacity, int gt_capacity);
size_t mvsdet_eval_workspace_bytes(int n_labels, int n_bound, int gt_capacity, int n_thr);
int mvsdet_eval_reset(void* state, size_t state_bytes, int n_labels, int capacity, int gt_capacity, mvsdet_stream_t stream);
int mvsdet_eval_match_f32(void* state, int n_labels, int capacity, int gt_capacity, const float* pred, const float* scores,
                          const int64_t* labels, const int* counts, int B, int Nmax, const float* gt, const int64_t* gt_labels,
                          const int* gt_counts, int G, int scene0, mvsdet_stream_t stream);
int mvsdet_eval_compute(const void* state, int n_labels, int capacity, int gt_capacity, int n_bound, const float* thresholds,
                        int n_thr, float* out_ap, double* out_recall, int* out_npos, int* out_ndet, int64_t* out_first,
                        unsigned char* out_tp, int* out_order, int* out_info, void* workspace, size_t workspace_bytes,
                        mvsdet_stream_t stream);
int mvsdet_eval_iou_f32(const float* a, int n, const float* b, int m, float* out, mvsdet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scores of the rendered target views of one scene (save_rendered_img_Image / save_rendered_depth of the reference's
 * nerf_utils/save_rendered_img.py, averaged as NVSMetric does; csrc/nvsmetric.hip) on the caller's stream, no host synchronisation,
 * no device allocation, no atomics; all arithmetic after the load is float64, and two runs give the same bits.
 *
 * State: MVSDET_NVS_STATE_DOUBLES float64 on the DEVICE, 8-byte aligned = {sum of the scenes' psnr, of their ssim, of their rmse,
 *   scenes}, cleared by mvsdet_nvs_reset.  NULL: nothing is accumulated.
 * mvsdet_nvs_score_f32: pred, gt = n_tgt x 3 x H x W float32 images in [0,1], each with HOST int64[4] element strides (view,
 *   channel, row, column) and read in place; pred_depth, gt_depth = n_tgt x H x W with HOST int64[3] strides, or both NULL.
 *   out_views (n_tgt,2) float64 = per view psnr = -10 log(mse) / log(10) (mse over the view's 3 H W elements; +inf for mse 0) and
 *   ssim = skimage's structural_similarity(channel_axis=-1, data_range=1): 7x7 box windows wholly inside the image, sample
 *   covariance, K1 = 0.01, K2 = 0.03, mean over the (H-6)(W-6) windows of a channel, then over the channels.  out_scene (3) float64 =
 *   the means over the views of psnr, ssim and of mean((pred_depth - gt_depth)^2) (the reference's "rmse": no root; 0 without a
 *   depth pair); they are added to the state with a scene count of 1.  pred = gt = NULL with a depth pair: out_scene = (0, 0, rmse),
 *   out_views is not written and state must be NULL.  Two launches.  H, W >= 7 and n_tgt * 3 * H * W < 2^31.
 *   Workspace: mvsdet_nvs_workspace_bytes(n_tgt, H, W, with_depth) (0: bad sizes), 8-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define MVSDET_NVS_STATE_DOUBLES 4
size_t mvsdet_nvs_workspace_bytes(int n_tgt, int H, int W, int with_depth);
int mvsdet_nvs_reset(double* state, mvsdet_stream_t stream);
int mvsdet_nvs_score_f32(double* state, const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                         const float* pred_depth, const int64_t* pred_depth_strides, const float* gt_depth,
                         const int64_t* gt_depth_strides, int n_tgt, int H, int W, double* out_views, double* out_scene,
                         void* workspace, size_t workspace_bytes, mvsdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVSDET_HIP_H */
