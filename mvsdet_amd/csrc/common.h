// Shared helpers of the mvsdet_hip library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/mvsdet_hip.h"

namespace mvsdet {

void set_error(const char* fmt, ...);

// Tuning options of the library: initialised ONCE from the environment (MVSDET_SWEEP_TW, _BOXCAP, _XCD, ...) the
// first time they are needed, afterwards changed only through mvsdet_set_option() -- no getenv on the launch path.
struct Options {
    int sweep_tw;      // 0 = by the map width, 16 / 32 force the tile shape (16x8 / 32x4)
    int sweep_boxcap;  // texels of one LDS footprint box (0 forces the global-gather path)
    int sweep_xcd;     // XCD-aware block map for fewer than 8 slabs
    int sweep_dsplit;  // 0 = by the grid size; n > 0: every block sweeps ceil(D / n) consecutive planes
    int sweep_groups;  // -1 = by the plane count; 0 / 1 = off; g in [2, kSweepGroups]: a tile's planes are dealt to up to g blocks,
                       // cut where its footprint boxes are refilled (the near planes)
    int conv_nsplit;   // bf16x3 convolutions: splits of the input channels; 0 = by the grid, n > 0 force (needs the workspace)
    int conv_xcd;      // stride-1 bf16x3 convolution: 1 (default) = an XCD takes a contiguous eighth of the grid (neighbouring tiles share
                       // their halo voxels in one L2); 0 = blocks round-robin over the XCDs
    int conv_split_blocks; // bf16x3 convolutions on small grids: the input channels are split until about this many blocks run (768 =
                       // three rounds of 256 CUs)
    int conv_split_min_groups; // ... and a split keeps at least this many groups of 8 input channels (default 2: neck + head 2.39 -> 2.35 ms against 4)
    int bwd_groups;    // backward sweep: wave groups of a block that share its gradient images and split its planes; 0 = by the plane
                       // count (2 from 32 planes), 1 / 2 force
    int sweep_inside;  // 1 (default) = planes whose taps all lie inside the image and the resident box (kFlagInside) take the slab kernel's
                       // lean decode; 0 = every plane takes the general decode (A/B runs, tests)
    int conv_mx_th;    // fp16 + MX convolution (costreg_mx.h): 0 (default) = wave-specialised kernel (8 multiplying + 4 staging waves, 4 x 8 x 16 tiles);
                       // 8 / 12 = every wave does everything on 4 x 8 x 16 (8 waves) / 4 x 12 x 16 (12 waves) tiles
    int sweep_pool;    // 1 (default) = mvsdet_plane_sweep_table_pooled_f32 builds the pooled geometry (K == 2, 32x4 tiles: a footprint box may
                       // take the other neighbour's idle LDS slot); 0 = it builds the geometry of mvsdet_plane_sweep_table_f32 (A/B runs, tests)
    int depthprob_ahead; // 1 (default) = depth_prob_topk requests a pixel's inputs before its first store (depth_prob_topk_ahead_kernel);
                       // 0 = the form that requests them plane by plane, behind the stores (A/B runs, tests).  Same bits.
    int sweep_store;   // cache policy of the sweep's output stores (FAST form, K == 2): kSweepStoreAuto (-1, default: what ships for the class) |
                       // kSweepStoreNt (0) | kSweepStorePlain | kSweepStoreSc1 | kSweepStoreSc0Sc1 | kSweepStoreNtSc1 | kSweepStoreNtBuffer.
                       // Only the flavours of MVS_SWEEP_STORE_LIST are compiled; set_option refuses the others.
                       // The store-pattern probe writes under the same policy.  Same bits under every value.
    int sweep_box_load; // cache policy of the footprint boxes' LDS-DMA and of a block's reference-feature loads: 0 (default) = default policy,
                       // 1 = non-temporal (MVS_SWEEP_LOAD_LIST).  Same bits.
    int pixel_dsplit;  // the per-pixel form (pixel_form.h: pixel_blocking): 0 = by the grid size; n > 0: every block walks ceil(D / min(n, D))
                       // consecutive hypotheses, the forward at most 4.  The forwards' bits do not depend on it (tests, A/B runs).
};
Options& options();

// Store flavours of option "sweep_store".  kSweepStoreNt is the non-temporal global store; the others are buffer stores whose aux
// operand carries the policy (gfx950: 0 plain, 1 sc0, 2 nt, 16 sc1, 17 sc0 sc1, 18 nt sc1).  kSweepStoreNtBuffer is the
// control of the A/B matrix: the policy of kSweepStoreNt through the other store instruction.
constexpr int kSweepStoreNt = 0, kSweepStorePlain = 1, kSweepStoreSc1 = 2, kSweepStoreSc0Sc1 = 3, kSweepStoreNtSc1 = 4, kSweepStoreNtBuffer = 5;
__host__ __device__ constexpr int sweep_store_aux(int st) {
    return st == kSweepStorePlain ? 0 : st == kSweepStoreSc1 ? 16 : st == kSweepStoreSc0Sc1 ? 17 : st == kSweepStoreNtSc1 ? 18 : 2;
}
constexpr int kSweepStoreAuto = -1;   // the option's default: per class of instantiation, what the A/B kept (sweep_store_shipped)
// What ships, per class (tile width, fp16 storage) -- the rule and the runs: profiles/r10_sweep_store_policy_ab.txt.  The 32x4 tiles with
// fp32 storage (the headline's class) passed with MVS_SWEEP_STORE_SHIPPED; the 16x8 tiles did not, and fp16 storage was not measured.
#define MVS_SWEEP_STORE_SHIPPED 4
constexpr int sweep_store_shipped(int tw, bool half) { return (tw == 32 && !half) ? MVS_SWEEP_STORE_SHIPPED : kSweepStoreNt; }
// What is compiled.  The A/B build (make SWEEP_STORE_MATRIX=1) carries every flavour on every class, for tools/sweep_store_policy_ab.py; the
// default build carries kSweepStoreNt everywhere and the shipped flavour on the class that ships it, and no load flavour but the default
// (non-temporal box loads lost 11 %).  X(value) per list; the slab kernel is instantiated on its FAST K == 2 forms.
#ifdef MVS_SWEEP_STORE_MATRIX
#define MVS_SWEEP_STORE_LIST(X) X(0) X(1) X(2) X(3) X(4) X(5)
#define MVS_SWEEP_LOAD_NT 1
constexpr bool sweep_class_has_flavours(int, bool) { return true; }
#else
#define MVS_SWEEP_STORE_LIST(X) X(0) X(MVS_SWEEP_STORE_SHIPPED)
#define MVS_SWEEP_LOAD_NT 0
constexpr bool sweep_class_has_flavours(int tw, bool half) { return sweep_store_shipped(tw, half) != kSweepStoreNt; }
#endif
#if MVS_SWEEP_LOAD_NT
#define MVS_SWEEP_LOAD_LIST(X) X(0) X(1)
#else
#define MVS_SWEEP_LOAD_LIST(X) X(0)
#endif
inline bool sweep_store_compiled(int v) {
#define MVS_X(S) if (v == S) return true;
    MVS_SWEEP_STORE_LIST(MVS_X)
#undef MVS_X
    return v == kSweepStoreAuto;
}
// The flavour a launch takes: the option, or under kSweepStoreAuto what ships for the class; kSweepStoreNt where the class has no other
// instantiation, or where the slab's 32 channel rows reach 4 GiB (a buffer store's offsets are 32 bits from the slab's base).
inline int sweep_store_for(int tw, bool half, size_t slab_bytes) {
    const int st = options().sweep_store == kSweepStoreAuto ? sweep_store_shipped(tw, half) : options().sweep_store;
    return (sweep_class_has_flavours(tw, half) && slab_bytes < ((size_t)1 << 32)) ? st : kSweepStoreNt;
}
inline bool sweep_box_load_compiled(int v) {
#define MVS_X(L) if (v == L) return true;
    MVS_SWEEP_LOAD_LIST(MVS_X)
#undef MVS_X
    return false;
}

// where plane_sweep_coords_kernel leaves the sweep geometry inside the scratch buffer (planesweep.hip)
struct SweepGeometry {
    int4* header;   // {kGeoMagic, tile width | (box capacity << 8), W, (D << 8) | K} written by plane_sweep_coords_kernel: the layout below hangs on the
                    // tile shape, so a consumer whose own choice differs (a pitched table fed to the contiguous call, another
                    // "sweep_tw") must not touch it -- the slab kernel checks the header and fills its output with NaN instead
    int4* boxes;
    unsigned* flags;
    float* proj;
    float* depth;
    unsigned short* groups;   // [N*tiles][kSweepGroups + 1] plane-group boundaries of every tile (sweep_kernel.h)
};
constexpr int kGeoMagic = 0x4d565347;   // "MVSG"
constexpr int kGeoMagicPooled = 0x4d565350;   // "MVSP": a geometry of the pooled run policy (mvsdet_plane_sweep_table_pooled_f32): boxes of more
                                              // texels than the capacity in the header live at the pool's base.  Only the forward slab kernel knows it.
constexpr int kSweepGroups = 6;   // at most this many plane groups (blocks) per (tile, slab)
SweepGeometry sweep_geometry(void* scratch, int N, int K, int D, int tiles);

constexpr int kWave = 64;       // CDNA wavefront
constexpr int kThreads = 256;   // 4 waves, one per SIMD
constexpr int kXcds = 8;        // MI355X: 8 XCDs, blocks are dealt round-robin over them

#define MVS_REQUIRE(cond, ...)              \
    do {                                    \
        if (!(cond)) {                      \
            ::mvsdet::set_error(__VA_ARGS__); \
            return MVSDET_ERR_INVALID_ARG;  \
        }                                   \
    } while (0)

// a helper's refusal (it has set the message) is the caller's
#define MVS_TRY(call)                           \
    do {                                        \
        if (const int rc_ = (call)) return rc_; \
    } while (0)

#define MVS_LAUNCH_CHECK(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            ::mvsdet::set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return MVSDET_ERR_HIP;                                                    \
        }                                                                             \
    } while (0)

// The one grant of dynamic LDS: a launch that needs more than 48 KiB has the kernel's limit raised to `ceiling`, a constant of the
// kernel -- never this call's own smaller need, which a second host thread with a larger one could find in force between its own
// grant and its launch.  On every launch, no "done" flag: the attribute is per device, and a process may drive several.  Host-side
// state only, nothing is enqueued: safe under stream capture.
template <class Kernel>
inline int grant_dynamic_lds(const char* name, Kernel* kernel, size_t need, size_t ceiling) {
    if (need <= 48 * 1024) return MVSDET_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ceiling) != hipSuccess) {
        set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed", name);
        return MVSDET_ERR_HIP;
    }
    return MVSDET_OK;
}
#define MVS_GRANT_LDS(name, kernel, need, ceiling) MVS_TRY(::mvsdet::grant_dynamic_lds(name, kernel, need, ceiling))

// A caller's buffer of `have` bytes where `need` are needed: the one wording of MVSDET_ERR_WORKSPACE, the operator's name first.
#define MVS_REQUIRE_WORKSPACE(name, have, need)                                                                        \
    do {                                                                                                               \
        if ((size_t)(have) < (size_t)(need)) {                                                                         \
            ::mvsdet::set_error("%s: workspace of %zu bytes, %zu needed", name, (size_t)(have), (size_t)(need));       \
            return MVSDET_ERR_WORKSPACE;                                                                               \
        }                                                                                                              \
    } while (0)

// blocks of kThreads threads for one thread per element
inline long long blocks_of(long long total) { return (total + kThreads - 1) / kThreads; }

// Blocks b and b+8 share an XCD (and its 4 MiB L2).  Map the hardware block id to a logical id so
// that every XCD walks ONE contiguous range of logical ids: neighbouring tiles of a view then find
// the source rows they share in their own L2.  Bijective for any nblocks (speed only, never
// correctness: MI355X_MICROARCH "Workgroup dispatch").
__device__ __forceinline__ int xcd_contiguous_id(int b, int nblocks) {
    const int q = nblocks / kXcds, r = nblocks % kXcds;
    const int xcd = b % kXcds, idx = b / kXcds;
    return (xcd < r) ? xcd * (q + 1) + idx : r * (q + 1) + (xcd - r) * q + idx;
}

// ---------------------------------------------------------------------------------------------
// Sampling taps of one (reference pixel, depth plane, source view): mvs_models/module.py:116-143 +
// ATen grid_sample(bilinear, zeros, align_corners=False).  Same rounding points as
// oracle/planesweep_oracle.c:orc_compute_taps (the library is compiled with -ffp-contract=off, so
// a fused multiply-add happens exactly where fmaf() is written).
//   P      proj = src_proj @ inverse(ref_proj), row-major 4x4
//   scale  element stride of one pixel in the sampled map (1 for NCHW planes, 4*G for packed maps)
//   off    element offsets of taps nw, ne, sw, se (0 for a tap outside the map)
//   w      bilinear weights (an outside tap carries weight*0, so Inf/NaN positions give NaN as ATen-CPU)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void compute_taps(const float* __restrict__ P, float x, float y, float d, int H, int W,
                                             int scale, int4& off, float4& w) {
    const float rx = fmaf(P[1], y, P[0] * x) + P[2];
    const float ry = fmaf(P[5], y, P[4] * x) + P[6];
    const float rz = fmaf(P[9], y, P[8] * x) + P[10];
    const float X = rx * d + P[3];
    const float Y = ry * d + P[7];
    const float Z = rz * d + P[11];
    const float px = X / Z;
    const float py = Y / Z;
    const float gx = px / ((float)(W - 1) * 0.5f) - 1.0f;
    const float gy = py / ((float)(H - 1) * 0.5f) - 1.0f;
    const float ix = fmaf(gx + 1.0f, (float)W * 0.5f, -0.5f);
    const float iy = fmaf(gy + 1.0f, (float)H * 0.5f, -0.5f);
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx = ix - x0, wy = iy - y0;
    const float ex = 1.0f - wx, sy = 1.0f - wy;
    const bool x0in = (x0 >= 0.0f) && (x0 <= (float)(W - 1));
    const bool x1in = (x0 >= -1.0f) && (x0 <= (float)(W - 2));
    const bool y0in = (y0 >= 0.0f) && (y0 <= (float)(H - 1));
    const bool y1in = (y0 >= -1.0f) && (y0 <= (float)(H - 2));
    const int xi = (x0in || x1in) ? (int)x0 : 0;
    const int yi = (y0in || y1in) ? (int)y0 : 0;
    const float wnw = sy * ex, wne = sy * wx, wsw = wy * ex, wse = wy * wx;
    const int base = yi * W + xi;
    off.x = (x0in && y0in) ? base * scale : 0;
    off.y = (x1in && y0in) ? (base + 1) * scale : 0;
    off.z = (x0in && y1in) ? (base + W) * scale : 0;
    off.w = (x1in && y1in) ? (base + W + 1) * scale : 0;
    w.x = (x0in && y0in) ? wnw : wnw * 0.0f;
    w.y = (x1in && y0in) ? wne : wne * 0.0f;
    w.z = (x0in && y1in) ? wsw : wsw * 0.0f;
    w.w = (x1in && y1in) ? wse : wse * 0.0f;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Voxel -> pixel projection of backproject_Weigh (mvsdet.py:1383-1391): q = P @ [p;1] summed in k
// order with fused multiply-adds (oracle: orc_project), x = round_half_even(q0/q2), valid test.
__device__ __forceinline__ bool project_voxel(const float* __restrict__ P, float px, float py, float pz, int h, int w,
                                              float& xr, float& yr, float& z) {
    const float q0 = fmaf(P[2], pz, fmaf(P[1], py, P[0] * px)) + P[3];
    const float q1 = fmaf(P[6], pz, fmaf(P[5], py, P[4] * px)) + P[7];
    const float q2 = fmaf(P[10], pz, fmaf(P[9], py, P[8] * px)) + P[11];
    xr = rintf(q0 / q2);
    yr = rintf(q1 / q2);
    z = q2;
    return (xr >= 0.0f) && (yr >= 0.0f) && (xr < (float)w) && (yr < (float)h) && (q2 > 0.0f);
}

// Depth window + weight of one (view, voxel) pair: mvsdet.py:1393-1428 (oracle: orc_depth_window).
// depth/dens point at view i; candidate j of pixel (yi,xi) is at [j*s1 + yi*s2 + xi*s3].
// Returns valid' and the weight max_j(m_j ? prob_norm_j : 0); *arg = index of the first maximal
// matching candidate (-1 if none has positive weight) for the backward pass.
__device__ __forceinline__ bool depth_window(const float* __restrict__ depth, const float* __restrict__ dens,
                                             int64_t s1, int64_t s2, int64_t s3, int J, int yi, int xi, float z,
                                             float vz, float& weight, float& psum_out, int& arg) {
    const int64_t base = (int64_t)yi * s2 + (int64_t)xi * s3;
    float psum = 0.0f;
    for (int j = 0; j < J; ++j) psum = psum + dens[base + j * s1];
    float wmax = 0.0f;
    bool any = false;
    int a = -1;
    for (int j = 0; j < J; ++j) {
        const float dj = depth[base + j * s1];
        const bool m = (z > dj - vz) && (z < dj + vz);
        const float pn = dens[base + j * s1] / psum;
        const float cand = m ? pn : 0.0f;
        if (cand > wmax) {
            wmax = cand;
            a = j;
        }
        if (cand != cand) wmax = cand;
        any = any || m;
    }
    weight = wmax;
    psum_out = psum;
    arg = a;
    return any;
}

}  // namespace mvsdet
