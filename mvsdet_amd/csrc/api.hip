// Library-level entry points: version, error string, HBM-ceiling copy kernel.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mvsdet {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// an option whose values select compiled instantiations: a value this build does not carry is named on stderr and not taken
static int env_compiled(const char* name, int dflt, bool (*compiled)(int)) {
    const int v = env_int(name, dflt);
    if (compiled(v)) return v;
    fprintf(stderr, "mvsdet: %s=%d is not compiled into this build; using %d\n", name, v, dflt);
    return dflt;
}

Options& options() {
    static Options o = {env_int("MVSDET_SWEEP_TW", 0), env_int("MVSDET_SWEEP_BOXCAP", 512), env_int("MVSDET_SWEEP_XCD", 1),
                        env_int("MVSDET_SWEEP_DSPLIT", 0), env_int("MVSDET_SWEEP_GROUPS", -1),
                        env_int("MVSDET_CONV_NSPLIT", 0), env_int("MVSDET_CONV_XCD", 1), env_int("MVSDET_CONV_SPLIT_BLOCKS", 768),
                        env_int("MVSDET_CONV_SPLIT_MIN_GROUPS", 2), env_int("MVSDET_BWD_GROUPS", 0), env_int("MVSDET_SWEEP_INSIDE", 1), env_int("MVSDET_CONV_MX_TH", 0),
                        env_int("MVSDET_SWEEP_POOL", 1), env_int("MVSDET_DEPTHPROB_AHEAD", 1),
                        env_compiled("MVSDET_SWEEP_STORE", kSweepStoreAuto, sweep_store_compiled), env_compiled("MVSDET_SWEEP_BOX_LOAD", 0, sweep_box_load_compiled),
                        env_int("MVSDET_PIXEL_DSPLIT", 0)};
    return o;
}

static int* option_slot(const char* name) {
    Options& o = options();
    if (!name) return nullptr;
    if (!strcmp(name, "sweep_tw")) return &o.sweep_tw;
    if (!strcmp(name, "sweep_boxcap")) return &o.sweep_boxcap;
    if (!strcmp(name, "sweep_xcd")) return &o.sweep_xcd;
    if (!strcmp(name, "sweep_dsplit")) return &o.sweep_dsplit;
    if (!strcmp(name, "pixel_dsplit")) return &o.pixel_dsplit;
    if (!strcmp(name, "sweep_groups")) return &o.sweep_groups;
    if (!strcmp(name, "sweep_inside")) return &o.sweep_inside;
    if (!strcmp(name, "sweep_pool")) return &o.sweep_pool;
    if (!strcmp(name, "sweep_store")) return &o.sweep_store;
    if (!strcmp(name, "sweep_box_load")) return &o.sweep_box_load;
    if (!strcmp(name, "depthprob_ahead")) return &o.depthprob_ahead;
    if (!strcmp(name, "conv_nsplit")) return &o.conv_nsplit;
    if (!strcmp(name, "conv_xcd")) return &o.conv_xcd;
    if (!strcmp(name, "bwd_groups")) return &o.bwd_groups;
    if (!strcmp(name, "conv_mx_th")) return &o.conv_mx_th;
    if (!strcmp(name, "conv_split_min_groups")) return &o.conv_split_min_groups;
    if (!strcmp(name, "conv_split_blocks")) return &o.conv_split_blocks;
    return nullptr;
}

// float4 grid-stride copy: the achievable-HBM yardstick of bench.py (MI355X_MICROARCH: 6.29 TB/s measured).
__global__ __launch_bounds__(kThreads) void copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
    // 4 independent 16-byte loads in flight per lane before the first store
    const size_t stride = (size_t)gridDim.x * kThreads;
    size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a;
        dst[i + stride] = b;
        dst[i + 2 * stride] = c;
        dst[i + 3 * stride] = d;
    }
    for (; i < n4; i += stride) dst[i] = src[i];
}

__global__ void copy_tail_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t begin, size_t n) {
    const size_t i = begin + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// The plane sweep's WRITE pattern alone (no taps, no LDS, no arithmetic): block = (view, TW x 128/TW pixel tile, 32-channel
// slab) loops over the planes; per plane each wave issues four non-temporal stores of 8 channel rows x 16 B per lane -- the
// block -> address map of plane_sweep_variance_kernel's FAST form on an (N,C,D,H,Wo) volume.  What this pattern reaches is the
// ceiling of the sweep's store stream on the box at hand (a device-to-device copy is not: DESIGN.md 4.1).
// ST: the store flavour of option "sweep_store", as in the slab kernel: kSweepStoreNt the non-temporal global store, any other a buffer
// store through a resource based at the block's slab.
template <int TW, typename OutT, int ST = kSweepStoreNt>
__global__ __launch_bounds__(kThreads) void store_pattern_kernel(OutT* __restrict__ var, int C, int D, int H, int W, int Wo,
                                                                  int tiles_x, int tiles, int d_per_block) {
    constexpr int TH = 128 / TW;
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    const int S = C / 32;
    const size_t HWo = (size_t)H * Wo;
    const int id = blockIdx.x;
    const int slab = id % S, bt = id / S;
    const int tile = bt % tiles, n = bt / tiles;
    const int tx0 = (tile % tiles_x) * TW, ty0 = (tile / tiles_x) * TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane & 7, ps = lane >> 3;
    const int p0 = 32 * wave + 4 * ps;
    const int px0 = tx0 + p0 % TW, py = ty0 + p0 / TW;
    if (py >= H || px0 + 4 > W) return;
    const size_t st_off = (size_t)py * Wo + px0;
    const v4f vv = {1.0f * id, 2.0f, 3.0f, (float)lane};
    const v2u hv = {(unsigned)id, (unsigned)lane};   // fp16 storage: the lane's 4 pixels are 8 bytes
    const int d0 = blockIdx.y * d_per_block, d1 = min(D, d0 + d_per_block);
    if constexpr (ST != kSweepStoreNt) {
        // the slab kernel's addressing: resource = the slab's 32 channel rows (below 4 GiB: checked by the entry point), scalar offset of
        // (plane, channel row 8*i), lane offset of (channel g, the pixels)
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        OutT* var_slab = var + ((size_t)n * C + slab * 32) * D * HWo;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(var_slab, 0, (int)(unsigned)((size_t)32 * D * HWo * sizeof(OutT)), 0x00020000);
        const unsigned l_off = (unsigned)(((size_t)g * D * HWo + st_off) * sizeof(OutT));
        const v4u uv = {(unsigned)id, 2u, 3u, (unsigned)lane};
        for (int d = d0; d < d1; ++d) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned s_off = (unsigned)(((size_t)d * HWo + (size_t)8 * i * D * HWo) * sizeof(OutT));
                if constexpr (sizeof(OutT) == 4) __builtin_amdgcn_raw_buffer_store_b128(uv, rsrc, (int)l_off, (int)s_off, sweep_store_aux(ST));
                else __builtin_amdgcn_raw_buffer_store_b64(hv, rsrc, (int)l_off, (int)s_off, sweep_store_aux(ST));
            }
        }
        return;
    }
    for (int d = d0; d < d1; ++d) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = slab * 32 + 8 * i + g;
            OutT* dst = var + (((size_t)n * C + c) * D + d) * HWo + st_off;
            if constexpr (sizeof(OutT) == 4) __builtin_nontemporal_store(vv, reinterpret_cast<v4f*>(dst));
            else __builtin_nontemporal_store(hv, reinterpret_cast<v2u*>(dst));
        }
    }
}

}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_version(void) { return 6003; }

template <typename OutT>
static int store_pattern_probe(OutT* var, int N, int C, int D, int H, int W, int out_w_pitch, int tile_w, int planes_per_block,
                               mvsdet_stream_t stream) {
    MVS_REQUIRE(var, "store_pattern_probe: NULL pointer");
    MVS_REQUIRE(N > 0 && C > 0 && C % 32 == 0 && D > 0 && H > 0 && W > 0 && W % 4 == 0, "store_pattern_probe: C %% 32 == 0 and W %% 4 == 0 wanted (the sweep's FAST form)");
    const int Wo = out_w_pitch > 0 ? out_w_pitch : W;
    MVS_REQUIRE(Wo >= W && Wo % 4 == 0 && ((uintptr_t)var % 16 == 0), "store_pattern_probe: pitch / alignment");
    MVS_REQUIRE(tile_w == 16 || tile_w == 32 || tile_w == 64, "store_pattern_probe: tile width 16, 32 or 64");
    const int th = 128 / tile_w;
    const int tiles_x = (W + tile_w - 1) / tile_w, tiles = tiles_x * ((H + th - 1) / th);
    const long long blocks = (long long)N * tiles * (C / 32);
    MVS_REQUIRE(blocks <= INT32_MAX, "store_pattern_probe: grid too large");
    const int dpb = planes_per_block > 0 ? std::min(planes_per_block, D) : D;
    dim3 grid((unsigned)blocks, (unsigned)((D + dpb - 1) / dpb));
    // the flavour the sweep takes for this tile shape, storage and volume ("sweep_store": common.h, sweep_store_for); 64-wide tiles have no
    // sweep: they follow the 32-wide ones
    const int st = sweep_store_for(tile_w == 16 ? 16 : 32, sizeof(OutT) == 2, (size_t)32 * D * H * Wo * sizeof(OutT));
#define MVS_PROBE(S)                                                                                                            \
    if (st == S) {                                                                                                              \
        if (tile_w == 16) hipLaunchKernelGGL((store_pattern_kernel<16, OutT, S>), grid, dim3(kThreads), 0, (hipStream_t)stream, var, C, D, H, W, Wo, tiles_x, tiles, dpb); \
        else if (tile_w == 64) hipLaunchKernelGGL((store_pattern_kernel<64, OutT, S>), grid, dim3(kThreads), 0, (hipStream_t)stream, var, C, D, H, W, Wo, tiles_x, tiles, dpb); \
        else hipLaunchKernelGGL((store_pattern_kernel<32, OutT, S>), grid, dim3(kThreads), 0, (hipStream_t)stream, var, C, D, H, W, Wo, tiles_x, tiles, dpb); \
    }
    MVS_SWEEP_STORE_LIST(MVS_PROBE)
#undef MVS_PROBE
    MVS_LAUNCH_CHECK("store_pattern_probe");
    return MVSDET_OK;
}

extern "C" int mvsdet_store_pattern_probe_f32(float* var, int N, int C, int D, int H, int W, int out_w_pitch, int tile_w,
                                              int planes_per_block, mvsdet_stream_t stream) {
    return store_pattern_probe(var, N, C, D, H, W, out_w_pitch, tile_w, planes_per_block, stream);
}

extern "C" int mvsdet_store_pattern_probe_f16(void* var, int N, int C, int D, int H, int W, int out_w_pitch, int tile_w,
                                              int planes_per_block, mvsdet_stream_t stream) {
    return store_pattern_probe(static_cast<unsigned short*>(var), N, C, D, H, W, out_w_pitch, tile_w, planes_per_block, stream);
}

extern "C" int mvsdet_set_option(const char* name, int value) {
    int* slot = option_slot(name);
    MVS_REQUIRE(slot, "set_option: unknown option '%s'", name ? name : "(null)");
    // these two select instantiations of the slab kernel: a flavour that this build does not carry is refused, never mapped to another
    MVS_REQUIRE(slot != &options().sweep_store || sweep_store_compiled(value), "set_option: sweep_store %d is not compiled into this build", value);
    MVS_REQUIRE(slot != &options().sweep_box_load || sweep_box_load_compiled(value), "set_option: sweep_box_load %d is not compiled into this build", value);
    *slot = value;
    return MVSDET_OK;
}

extern "C" int mvsdet_validate_neighbors(const int64_t* nbr, int M, int K, int n_src) {
    MVS_REQUIRE(M >= 0 && K >= 0 && n_src > 0, "validate_neighbors: bad shape M=%d K=%d n_src=%d", M, K, n_src);
    MVS_REQUIRE(K == 0 || M == 0 || nbr, "validate_neighbors: NULL pointer");
    for (int m = 0; m < M; ++m)
        for (int j = 0; j < K; ++j) {
            const int64_t v = nbr[(size_t)m * K + j];
            MVS_REQUIRE(v >= 0 && v < n_src, "neighbour id %lld of view %d (slot %d) outside [0, %d)", (long long)v, m, j, n_src);
        }
    return MVSDET_OK;
}

extern "C" int mvsdet_get_option(const char* name, int* value) {
    int* slot = option_slot(name);
    MVS_REQUIRE(slot && value, "get_option: unknown option '%s'", name ? name : "(null)");
    *value = *slot;
    return MVSDET_OK;
}

extern "C" const char* mvsdet_last_error(void) { return g_err; }

extern "C" int mvsdet_copy_f32(const float* src, float* dst, size_t n, mvsdet_stream_t stream) {
    MVS_REQUIRE(src && dst, "copy: NULL pointer");
    MVS_REQUIRE(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0), "copy: pointers must be 16-byte aligned");
    const size_t n4 = n / 4;
    if (n4) {
        const size_t want = (n4 + kThreads - 1) / kThreads;
        const unsigned grid = (unsigned)(want < 2048 ? want : 2048);  // 256 CUs x 8 blocks, grid-stride the rest
        hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, (const float4*)src, (float4*)dst, n4);
    }
    if (n % 4) hipLaunchKernelGGL(copy_tail_kernel, dim3(1), dim3(4), 0, (hipStream_t)stream, src, dst, n4 * 4, n);
    MVS_LAUNCH_CHECK("copy");
    return MVSDET_OK;
}
