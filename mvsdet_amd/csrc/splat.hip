// Gaussian rasteriser (Kerbl et al. 2023, with spherical harmonics up to degree 4): what gs_src/model/decoder/cuda_splatting.py::
// render_cuda asks of its external extension, for V views that share one set of G Gaussians.  DESIGN.md 4.15.
//
//   cameras     one thread per view: the matrices render_cuda builds, float64 inside, rounded once
//   preprocess  one thread per (view, Gaussian): cull, 2-D covariance, conic, radius, tile rectangle, colour
//   scan        one block per view: where each Gaussian's keys start; the needed key count goes to the status word
//   emit        one key (view-tile | depth) per (Gaussian, tile), value = the key's own position; padding keys sort last
//   sort        rocPRIM's device radix sort (stable: equal depths keep the Gaussians' index order)
//   ranges      first / last sorted entry of every tile
//   render      one block per (tile, view), the list staged through LDS in batches of 256
//   render bwd  the same walk back to front; every (tile, Gaussian) entry is reduced over the tile's pixels inside the block and
//               written to the slot of the key's pre-sort position
//   preprocess bwd  one thread per Gaussian adds its slots in tile order, then view order, and chains to the inputs
// fp32, no float atomics, no host synchronisation: two runs give the same bits.
//
// Rendered depth (render_depth_cuda) is a fourth blended channel of the same pass: preprocess writes one value d(v, g)
// per (view, Gaussian) -- the camera-space z mapped by the mode -- and render / render bwd / preprocess bwd are templates over
// "blends colour" and "blends depth".  Colour alone is the form above, unchanged; the two entry points choose the form by two flags.
#include <cstring>   // rocPRIM calls the host memset without including it

#include <rocprim/rocprim.hpp>

#include <climits>

#include "block_reduce.h"
#include "camera_math.h"
#include "sh_basis.h"

namespace mvsdet {
namespace {

constexpr int kTile = 16;
constexpr int kCam = 40;         // floats per view: view matrix 16, full projection 16, tan fov x / y, camera position 3, scale, 2 unused
constexpr int kSlot = 9;         // floats per (tile, Gaussian) gradient slot: mean2D 2, conic 3, opacity 1, colour 3
constexpr int kSlotDepth = 10;   // the depth forms' slot: the same nine (colour unused without colour) and dL/dd
constexpr int kBwdBatch = 64;    // entries of a tile list per LDS batch of the backward
constexpr unsigned kPadTile = 0xffffffffu;

struct SplatIn {
    const float* means;
    int64_t m_g, m_c;
    const float* cov;
    int64_t c_g, c_r, c_c;
    const float* sh;
    int64_t s_g, s_ch, s_k;
    const float* opac;
    int64_t o_g;
};

struct SplatWs {
    int4* status;        // V: {needed keys (saturated), capacity, overflow, 0}
    int* radii;          // V*G: radius in pixels, 0 = culled (second block of the workspace: ops.splat.radii reads it)
    float* depth;        // V*G
    float2* xy;          // V*G
    float4* conop;       // V*G
    float* rgb;          // V*G*3
    int4* rect;          // V*G: tile rectangle {x0, y0, x1, y1}, empty = culled
    unsigned* offs;      // V*G
    unsigned* touched;   // V*G
    uint64_t* keys_in;   // V*K
    uint64_t* keys_out;  // V*K
    unsigned* vals_in;   // V*K
    unsigned* vals_out;  // V*K
    unsigned* gid;       // V*K: Gaussian of the key at a pre-sort position
    int2* ranges;        // V*tiles
    float* final_T;      // V*H*W
    int* n_contrib;      // V*H*W
    void* sort_tmp;
    size_t sort_bytes;
    size_t total;
};

// The depth forms' extra arguments; an empty struct in the colour-only form, whose kernels keep their argument lists.
enum { kModeDepth = 0, kModeDisparity = 1, kModeRelativeDisparity = 2, kModeLog = 3 };
template <bool DEP>
struct SplatDepth {};
template <>
struct SplatDepth<true> {
    const float* near;     // V, unscaled
    const float* far;      // V, unscaled
    float* values;         // V*G: d(v, g), 0 where culled (the reference's fake_color)
    float* image;          // V*H*W: the rendered depth (forward) or its gradient (backward, read only)
    int mode;
};

// slots of the gradient record a form reduces and adds: the colour slots 6..8 are skipped without colour
template <bool COL>
__device__ __forceinline__ constexpr bool splat_slot_used(int k) {
    return COL || k < 6 || k > 8;
}

// d(z) of render_depth_cuda (cuda_splatting.py:253-262) and its derivative, fp32 in the reference's order of operations.  z is the
// camera-space depth before the scale_invariant scaling; near / far are the caller's, unscaled.
// The log mode's clamp is inverted in the reference -- min with near, then max with far -- so the value is log(far) for every
// Gaussian whenever near <= far, and its derivative in z is 0.  Reproduced as written, not corrected.
__device__ __forceinline__ float splat_depth_value(int mode, float z, float near, float far) {
    if (mode == kModeDisparity) return 1.0f / z;
    if (mode == kModeRelativeDisparity) {
        const float e = 1e-10f;
        const float disp_near = 1.0f / (near + e), disp_far = 1.0f / (far + e), disp = 1.0f / (z + e);
        return 1.0f - (disp - disp_far) / (disp_near - disp_far + e);
    }
    // the logarithm through float64, rounded once: the value is one number per view (log(far)), and a last-bit difference between two
    // float32 log routines would show in every pixel
    if (mode == kModeLog) return (float)log((double)fmaxf(fminf(z, near), far));
    return z;
}
__device__ __forceinline__ float splat_depth_slope(int mode, float z, float near, float far) {
    if (mode == kModeDisparity) return -1.0f / (z * z);
    if (mode == kModeRelativeDisparity) {
        const float e = 1e-10f;
        const float disp_near = 1.0f / (near + e), disp_far = 1.0f / (far + e), disp = 1.0f / (z + e);
        return disp * disp / (disp_near - disp_far + e);
    }
    if (mode == kModeLog) return 0.0f;
    return 1.0f;
}

// bits of the key above the depth: real (view, tile) ids stay below the padding key's all-ones field
unsigned tile_bits(int V, size_t tiles) {
    unsigned bits = 0;
    while (((unsigned long long)V * tiles) >> bits) ++bits;
    return bits;
}

// What rocPRIM's radix sort of n (64-bit key, 32-bit value) pairs may ask for: a second copy of keys and values plus its histograms and
// look-back states.  A fixed formula, so the workspace size does not hang on a device query; the forward checks the real need against it.
size_t sort_temp_bytes(size_t n) { return 16 * n + (1u << 20); }

SplatWs splat_layout(void* base, int V, int G, int H, int W, int K) {
    SplatWs ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = (char*)base + off;
        off += (bytes + 255) / 256 * 256;
        return (void*)p;
    };
    const size_t vg = (size_t)V * G, vk = (size_t)V * K, px = (size_t)V * H * W;
    const size_t tiles = (size_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    ws.status = (int4*)take(V * sizeof(int4));
    ws.radii = (int*)take(vg * 4);
    ws.depth = (float*)take(vg * 4);
    ws.xy = (float2*)take(vg * 8);
    ws.conop = (float4*)take(vg * 16);
    ws.rgb = (float*)take(vg * 12);
    ws.rect = (int4*)take(vg * 16);
    ws.offs = (unsigned*)take(vg * 4);
    ws.touched = (unsigned*)take(vg * 4);
    ws.keys_in = (uint64_t*)take(vk * 8);
    ws.keys_out = (uint64_t*)take(vk * 8);
    ws.vals_in = (unsigned*)take(vk * 4);
    ws.vals_out = (unsigned*)take(vk * 4);
    ws.gid = (unsigned*)take(vk * 4);
    ws.ranges = (int2*)take(V * tiles * 8);
    ws.final_T = (float*)take(px * 4);
    ws.n_contrib = (int*)take(px * 4);
    ws.sort_bytes = sort_temp_bytes(vk);
    ws.sort_tmp = take(ws.sort_bytes);
    ws.total = off;
    return ws;
}

// ------------------------------------------------------------------------------------------------ cameras
__global__ void splat_cameras_kernel(const float* __restrict__ ext, int64_t e_view, const float* __restrict__ kin, int64_t k_view,
                                     int64_t k_row, const float* __restrict__ near, const float* __restrict__ far, int scale_invariant,
                                     float* __restrict__ cams, int V) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* E = ext + v * e_view;
    const float* Kp = kin + v * k_view;
    float* c = cams + (int64_t)v * kCam;
    // render_cuda's own fp32 steps: scale = 1 / near, translation * scale, near * scale, far * scale
    const float s = scale_invariant ? 1.0f / near[v] : 1.0f;
    const float tr[3] = {scale_invariant ? E[3] * s : E[3], scale_invariant ? E[7] * s : E[7], scale_invariant ? E[11] * s : E[11]};
    const double n = scale_invariant ? (double)(near[v] * s) : (double)near[v];
    const double f = scale_invariant ? (double)(far[v] * s) : (double)far[v];
    // world-to-camera = inverse of [A | t; 0 0 0 1] by the adjugate of A
    double A[3][3], K[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[i][j] = (double)E[i * 4 + j];
            K[i][j] = (double)Kp[i * k_row + j];
        }
    double R[3][3], Ki[3][3], T[3];
    inverse3(A, R);
    inverse3(K, Ki);
    for (int i = 0; i < 3; ++i) T[i] = -(R[i][0] * (double)tr[0] + R[i][1] * (double)tr[1] + R[i][2] * (double)tr[2]);
    // field of view (gs_src/geometry/projection.py::get_fov): the angle between the unprojected edge midpoints
    auto unproject = [&](double x, double y, double* o) {
        for (int i = 0; i < 3; ++i) o[i] = Ki[i][0] * x + Ki[i][1] * y + Ki[i][2];
        const double len = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
        for (int i = 0; i < 3; ++i) o[i] /= len;
    };
    double l[3], r[3], t[3], b[3];
    unproject(0.0, 0.5, l);
    unproject(1.0, 0.5, r);
    unproject(0.5, 0.0, t);
    unproject(0.5, 1.0, b);
    const double tanx = tan(0.5 * acos(l[0] * r[0] + l[1] * r[1] + l[2] * r[2]));
    const double tany = tan(0.5 * acos(t[0] * b[0] + t[1] * b[1] + t[2] * b[2]));
    // row-vector forms: view[i][j] = W2C[j][i]; projection (get_projection_matrix) transposed; full = view @ projection
    double VMd[4][4], PT[4][4] = {};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) VMd[i][j] = R[j][i];
        VMd[3][i] = T[i];
        VMd[i][3] = 0.0;
    }
    VMd[3][3] = 1.0;
    PT[0][0] = 1.0 / tanx;          // 2 near / (right - left)
    PT[1][1] = 1.0 / tany;
    PT[2][2] = f / (f - n);
    PT[3][2] = -(f * n) / (f - n);  // P[2][3]
    PT[2][3] = 1.0;                 // P[3][2]
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += VMd[i][k] * PT[k][j];
            c[i * 4 + j] = (float)VMd[i][j];
            c[16 + i * 4 + j] = (float)acc;
        }
    c[32] = (float)tanx;
    c[33] = (float)tany;
    c[34] = tr[0];
    c[35] = tr[1];
    c[36] = tr[2];
    c[37] = s;
    c[38] = 0.0f;
    c[39] = 0.0f;
}

// ------------------------------------------------------------------------------------------------ projection of one Gaussian
struct Geo {
    float m[3];    // mean * scale
    float S[6];    // covariance * scale^2: 00 01 02 11 12 22
    float t[3];    // camera space
    float txc, tyc;
    bool clx, cly;
    float hx, hy, hw, pw;
    float J00, J02, J11, J12;
    float M0[3], M1[3];    // rows of J R
    float SM0[3], SM1[3];  // Sigma M0^T, Sigma M1^T
    float a, b, c, det;
};

// false: culled (behind the near bound 0.2, a NaN depth, or a singular / NaN 2-D covariance)
__device__ __forceinline__ bool splat_project(const float* __restrict__ cam, const SplatIn& in, int g, int H, int W, Geo& q) {
    const float s = cam[37], s2 = s * s;
    for (int i = 0; i < 3; ++i) q.m[i] = in.means[g * in.m_g + i * in.m_c] * s;
    for (int j = 0; j < 3; ++j) q.t[j] = q.m[0] * cam[j] + q.m[1] * cam[4 + j] + q.m[2] * cam[8 + j] + cam[12 + j];
    if (!(q.t[2] > 0.2f)) return false;
    const float* P = cam + 16;
    q.hx = q.m[0] * P[0] + q.m[1] * P[4] + q.m[2] * P[8] + P[12];
    q.hy = q.m[0] * P[1] + q.m[1] * P[5] + q.m[2] * P[9] + P[13];
    q.hw = q.m[0] * P[3] + q.m[1] * P[7] + q.m[2] * P[11] + P[15];
    q.pw = 1.0f / (q.hw + 1e-7f);
    const float* C = in.cov + g * in.c_g;
    q.S[0] = C[0] * s2;
    q.S[1] = C[in.c_c] * s2;
    q.S[2] = C[2 * in.c_c] * s2;
    q.S[3] = C[in.c_r + in.c_c] * s2;
    q.S[4] = C[in.c_r + 2 * in.c_c] * s2;
    q.S[5] = C[2 * in.c_r + 2 * in.c_c] * s2;
    const float tanx = cam[32], tany = cam[33];
    const float limx = 1.3f * tanx, limy = 1.3f * tany;
    const float tz = q.t[2];
    const float rx = q.t[0] / tz, ry = q.t[1] / tz;
    q.clx = (rx < -limx) || (rx > limx);
    q.cly = (ry < -limy) || (ry > limy);
    q.txc = fminf(limx, fmaxf(-limx, rx)) * tz;
    q.tyc = fminf(limy, fmaxf(-limy, ry)) * tz;
    const float fx = (float)W / (2.0f * tanx), fy = (float)H / (2.0f * tany);
    q.J00 = fx / tz;
    q.J02 = -(fx * q.txc) / (tz * tz);
    q.J11 = fy / tz;
    q.J12 = -(fy * q.tyc) / (tz * tz);
    for (int i = 0; i < 3; ++i) {
        q.M0[i] = q.J00 * cam[i * 4 + 0] + q.J02 * cam[i * 4 + 2];
        q.M1[i] = q.J11 * cam[i * 4 + 1] + q.J12 * cam[i * 4 + 2];
    }
    const float* S = q.S;
    q.SM0[0] = S[0] * q.M0[0] + S[1] * q.M0[1] + S[2] * q.M0[2];
    q.SM0[1] = S[1] * q.M0[0] + S[3] * q.M0[1] + S[4] * q.M0[2];
    q.SM0[2] = S[2] * q.M0[0] + S[4] * q.M0[1] + S[5] * q.M0[2];
    q.SM1[0] = S[0] * q.M1[0] + S[1] * q.M1[1] + S[2] * q.M1[2];
    q.SM1[1] = S[1] * q.M1[0] + S[3] * q.M1[1] + S[4] * q.M1[2];
    q.SM1[2] = S[2] * q.M1[0] + S[4] * q.M1[1] + S[5] * q.M1[2];
    q.a = q.M0[0] * q.SM0[0] + q.M0[1] * q.SM0[1] + q.M0[2] * q.SM0[2] + 0.3f;
    q.b = q.M0[0] * q.SM1[0] + q.M0[1] * q.SM1[1] + q.M0[2] * q.SM1[2];
    q.c = q.M1[0] * q.SM1[0] + q.M1[1] * q.SM1[1] + q.M1[2] * q.SM1[2] + 0.3f;
    q.det = q.a * q.c - q.b * q.b;
    return fabsf(q.det) > 0.0f;
}

// unit direction from the camera to the (scaled) mean; len = its length before normalising
__device__ __forceinline__ void splat_direction(const float* __restrict__ cam, const float* m, float* n, float& len) {
    const float dx = m[0] - cam[34], dy = m[1] - cam[35], dz = m[2] - cam[36];
    len = sqrtf(dx * dx + dy * dy + dz * dz);
    n[0] = dx / len;
    n[1] = dy / len;
    n[2] = dz / len;
}

// ------------------------------------------------------------------------------------------------ preprocess
template <bool COL, bool DEP>
__global__ __launch_bounds__(kThreads) void splat_preprocess_kernel(SplatIn in, const float* __restrict__ cams, SplatWs ws, int V, int G,
                                                                    int d_sh, int use_sh, int H, int W, int tiles_x, int tiles_y,
                                                                    SplatDepth<DEP> dz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V * G) return;
    const int v = i / G, g = i - v * G;
    const float* cam = cams + (int64_t)v * kCam;
    ws.rect[i] = make_int4(0, 0, 0, 0);
    ws.radii[i] = 0;
    ws.touched[i] = 0u;
    ws.depth[i] = 0.0f;
    ws.xy[i] = make_float2(0.0f, 0.0f);
    ws.conop[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (COL) ws.rgb[i * 3 + 0] = ws.rgb[i * 3 + 1] = ws.rgb[i * 3 + 2] = 0.0f;
    if constexpr (DEP) dz.values[i] = 0.0f;
    Geo q;
    if (!splat_project(cam, in, g, H, W, q)) return;
    const float mid = 0.5f * (q.a + q.c);
    const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - q.det));
    const float radius = ceilf(3.0f * sqrtf(lam));
    const float px = ((q.hx * q.pw + 1.0f) * (float)W - 1.0f) * 0.5f;
    const float py = ((q.hy * q.pw + 1.0f) * (float)H - 1.0f) * 0.5f;
    // clamped in float before the conversion: the same integers as clamp(int(.), 0, grid) for every finite value, 0 for NaN
    const float gx = (float)tiles_x, gy = (float)tiles_y, ft = (float)kTile;
    const int x0 = (int)fminf(fmaxf((px - radius) / ft, 0.0f), gx), x1 = (int)fminf(fmaxf((px + radius + (ft - 1.0f)) / ft, 0.0f), gx);
    const int y0 = (int)fminf(fmaxf((py - radius) / ft, 0.0f), gy), y1 = (int)fminf(fmaxf((py + radius + (ft - 1.0f)) / ft, 0.0f), gy);
    if (x1 <= x0 || y1 <= y0) return;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (!COL) {
        // depth alone: the harmonics are not read
    } else if (use_sh) {
        float n[3], len, basis[kShMax];
        splat_direction(cam, q.m, n, len);
        sh_basis<float>(n[0], n[1], n[2], d_sh, basis);
        for (int ch = 0; ch < 3; ++ch) {
            const float* sh = in.sh + g * in.s_g + ch * in.s_ch;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < kShMax; ++k)
                if (k < d_sh) acc += basis[k] * sh[k * in.s_k];
            acc += 0.5f;
            rgb[ch] = acc < 0.0f ? 0.0f : acc;
        }
    } else {
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = in.sh[g * in.s_g + ch * in.s_ch];
    }
    ws.rect[i] = make_int4(x0, y0, x1, y1);
    ws.radii[i] = (int)fminf(radius, 2147483520.0f);
    ws.touched[i] = (unsigned)((x1 - x0) * (y1 - y0));
    ws.depth[i] = q.t[2];
    ws.xy[i] = make_float2(px, py);
    ws.conop[i] = make_float4(q.c / q.det, -q.b / q.det, q.a / q.det, in.opac[g * in.o_g]);
    if constexpr (COL) {
        ws.rgb[i * 3 + 0] = rgb[0];
        ws.rgb[i * 3 + 1] = rgb[1];
        ws.rgb[i * 3 + 2] = rgb[2];
    }
    // the unscaled camera-space z as z_s / s: the scaled form above keeps its multiplication order (sort keys and culling do not
    // move), and with scale 1 the division is exact
    if constexpr (DEP) dz.values[i] = splat_depth_value(dz.mode, q.t[2] / cam[37], dz.near[v], dz.far[v]);
}

// one block per view: exclusive sums of `touched` in Gaussian order
__global__ __launch_bounds__(kThreads) void splat_scan_kernel(SplatWs ws, int G, int K) {
    __shared__ unsigned long long part[kThreads];
    const int v = blockIdx.x, t = threadIdx.x;
    const int chunk = (G + kThreads - 1) / kThreads;
    const int lo = min(t * chunk, G), hi = min(lo + chunk, G);
    const unsigned* touched = ws.touched + (size_t)v * G;
    unsigned long long sum = 0;
    for (int g = lo; g < hi; ++g) sum += touched[g];
    part[t] = sum;
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {
        const unsigned long long add = t >= step ? part[t - step] : 0ull;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned long long run = part[t] - sum;
    const unsigned long long total = part[kThreads - 1];
    const bool over = total > (unsigned long long)K;
    unsigned* offs = ws.offs + (size_t)v * G;
    for (int g = lo; g < hi; ++g) {
        offs[g] = over ? 0u : (unsigned)run;
        run += touched[g];
    }
    if (t == 0) ws.status[v] = make_int4((int)(total > (unsigned long long)INT_MAX ? (unsigned long long)INT_MAX : total), K, over ? 1 : 0, 0);
}

__global__ __launch_bounds__(kThreads) void splat_emit_kernel(SplatWs ws, int V, int G, int K, int tiles_x, int tiles) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = first; i < (int64_t)V * G; i += stride) {
        const int v = (int)(i / G), g = (int)(i - (int64_t)v * G);
        const int4 st = ws.status[v];
        const unsigned n = ws.touched[i];
        if (st.z || n == 0u) continue;
        const int4 r = ws.rect[i];
        const unsigned o = ws.offs[i];
        if ((unsigned long long)o + n > (unsigned long long)K) continue;   // cannot happen when the view fits; never write past the view
        const uint64_t depth = (uint64_t)__float_as_uint(ws.depth[i]);
        unsigned p = (unsigned)v * (unsigned)K + o;
        for (int y = r.y; y < r.w; ++y)
            for (int x = r.x; x < r.z; ++x, ++p) {
                ws.keys_in[p] = ((uint64_t)((unsigned)v * (unsigned)tiles + (unsigned)(y * tiles_x + x)) << 32) | depth;
                ws.vals_in[p] = p;
                ws.gid[p] = (unsigned)g;
            }
    }
    for (int64_t p = first; p < (int64_t)V * K; p += stride) {
        const int v = (int)(p / K);
        const int4 st = ws.status[v];
        const int valid = st.z ? 0 : st.x;
        if ((int)(p - (int64_t)v * K) >= valid) {
            ws.keys_in[p] = ~0ull;
            ws.vals_in[p] = (unsigned)p;
            ws.gid[p] = 0u;
        }
    }
}

__global__ __launch_bounds__(kThreads) void splat_ranges_kernel(SplatWs ws, int64_t n, unsigned all_tiles) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned t = (unsigned)(ws.keys_out[i] >> 32);
    if (t == kPadTile || t >= all_tiles) return;
    if (i == 0 || (unsigned)(ws.keys_out[i - 1] >> 32) != t) ws.ranges[t].x = (int)i;
    if (i == n - 1 || (unsigned)(ws.keys_out[i + 1] >> 32) != t) ws.ranges[t].y = (int)(i + 1);
}

// ------------------------------------------------------------------------------------------------ render
// alpha of a Gaussian at a pixel, capped at 0.99.  A comparison, not fminf: fminf returns its non-NaN argument, which would paint a
// Gaussian of NaN opacity as an opaque 0.99 layer and show no NaN; this keeps it.  The same value for every other input.
__device__ __forceinline__ float splat_alpha(float opacity, float gauss) {
    const float a = opacity * gauss;
    return a > 0.99f ? 0.99f : a;
}

// COL: blends the three colour channels into image (V,3,H,W) over the background.  DEP: blends d(v, g) into dz.image (V,H,W) over a
// background of 0, with the same alpha, T, skips, early stop and n_contrib.  Without COL no colour is staged in LDS.
template <bool COL, bool DEP>
__global__ __launch_bounds__(kThreads) void splat_render_kernel(SplatWs ws, const float* __restrict__ bg, float* __restrict__ image, int G,
                                                                int H, int W, int tiles_x, int tiles, SplatDepth<DEP> dz) {
    __shared__ float2 s_xy[kThreads];
    __shared__ float4 s_con[kThreads];
    __shared__ float s_rgb[COL ? kThreads * 3 : 1];
    __shared__ float s_d[DEP ? kThreads : 1];
    const int v = blockIdx.z, tid = threadIdx.x;
    const int px = blockIdx.x * kTile + (tid & (kTile - 1)), py = blockIdx.y * kTile + (tid >> 4);
    const bool inside = px < W && py < H;
    const int64_t pix = ((int64_t)v * H + py) * W + px;
    const int64_t plane = (int64_t)H * W;
    float* out = image + (int64_t)v * 3 * plane + (int64_t)py * W + px;
    if (ws.status[v].z) {   // more keys than the capacity: the view is NaN, nothing was sorted for it
        if (inside) {
            const float nan = __builtin_nanf("");
            if constexpr (COL) out[0] = out[plane] = out[2 * plane] = nan;
            if constexpr (DEP) dz.image[pix] = nan;
            ws.final_T[pix] = nan;
            ws.n_contrib[pix] = 0;
        }
        return;
    }
    const int2 range = ws.ranges[v * tiles + blockIdx.y * tiles_x + blockIdx.x];
    const int n = range.y - range.x;
    const float fx = (float)px, fy = (float)py;
    float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, D = 0.0f;
    int contributor = 0, last = 0;
    bool done = !inside;
    for (int base = 0; base < n; base += kThreads) {
        if (__syncthreads_count(done) == kThreads) break;
        if (base + tid < n) {
            const unsigned p = ws.vals_out[range.x + base + tid];
            const size_t gi = (size_t)v * G + ws.gid[p];
            s_xy[tid] = ws.xy[gi];
            s_con[tid] = ws.conop[gi];
            if constexpr (COL) {
                s_rgb[tid * 3 + 0] = ws.rgb[gi * 3 + 0];
                s_rgb[tid * 3 + 1] = ws.rgb[gi * 3 + 1];
                s_rgb[tid * 3 + 2] = ws.rgb[gi * 3 + 2];
            }
            if constexpr (DEP) s_d[tid] = dz.values[gi];
        }
        __syncthreads();
        const int m = min(kThreads, n - base);
        for (int j = 0; j < m && !done; ++j) {
            ++contributor;
            const float2 xy = s_xy[j];
            const float4 co = s_con[j];
            const float dx = xy.x - fx, dy = xy.y - fy;
            const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
            if (power > 0.0f) continue;
            const float alpha = splat_alpha(co.w, expf(power));
            if (alpha < 1.0f / 255.0f) continue;
            const float Tn = T * (1.0f - alpha);
            if (Tn < 0.0001f) {
                done = true;
                continue;
            }
            const float w = alpha * T;
            if constexpr (COL) {
                C0 += s_rgb[j * 3 + 0] * w;
                C1 += s_rgb[j * 3 + 1] * w;
                C2 += s_rgb[j * 3 + 2] * w;
            }
            if constexpr (DEP) D += s_d[j] * w;
            T = Tn;
            last = contributor;
        }
    }
    if (inside) {
        if constexpr (COL) {
            out[0] = C0 + T * bg[v * 3 + 0];
            out[plane] = C1 + T * bg[v * 3 + 1];
            out[2 * plane] = C2 + T * bg[v * 3 + 2];
        }
        if constexpr (DEP) dz.image[pix] = D;
        ws.final_T[pix] = T;
        ws.n_contrib[pix] = last;
    }
}

// DEP: g_depth (dz.image) enters the recurrence as one more channel with its own accum / last pair and no background term; the slot
// has kSlotDepth floats, the last one dL/dd.  Without COL the colour slots 6..8 are neither reduced nor written.
template <bool COL, bool DEP>
__global__ __launch_bounds__(kThreads) void splat_render_bwd_kernel(SplatWs ws, const float* __restrict__ bg, const float* __restrict__ g_image,
                                                                    float* __restrict__ slots, int G, int H, int W, int tiles_x, int tiles,
                                                                    SplatDepth<DEP> dz) {
    constexpr int NS = DEP ? kSlotDepth : kSlot;
    __shared__ float2 s_xy[kBwdBatch];
    __shared__ float4 s_con[kBwdBatch];
    __shared__ float s_rgb[COL ? kBwdBatch * 3 : 1];
    __shared__ float s_d[DEP ? kBwdBatch : 1];
    __shared__ unsigned s_pos[kBwdBatch];
    __shared__ float s_part[kThreads / kWave][kBwdBatch][NS];
    const int v = blockIdx.z, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    if (ws.status[v].z) return;   // nothing was sorted for this view; preprocess backward writes its NaN
    const int px = blockIdx.x * kTile + (tid & (kTile - 1)), py = blockIdx.y * kTile + (tid >> 4);
    const bool inside = px < W && py < H;
    const int64_t pix = ((int64_t)v * H + py) * W + px;
    const int64_t plane = (int64_t)H * W;
    const int2 range = ws.ranges[v * tiles + blockIdx.y * tiles_x + blockIdx.x];
    const int n = range.y - range.x;
    const float fx = (float)px, fy = (float)py;
    const float T_final = inside ? ws.final_T[pix] : 0.0f;
    const int last = inside ? ws.n_contrib[pix] : 0;
    float dp[3] = {0.0f, 0.0f, 0.0f};
    float bg_dot = 0.0f;
    if constexpr (COL) {
        if (inside)
            for (int ch = 0; ch < 3; ++ch) dp[ch] = g_image[(int64_t)v * 3 * plane + ch * plane + (int64_t)py * W + px];
        bg_dot = bg[v * 3 + 0] * dp[0] + bg[v * 3 + 1] * dp[1] + bg[v * 3 + 2] * dp[2];
    }
    float dpd = 0.0f, accum_d = 0.0f, last_d = 0.0f;
    if constexpr (DEP)
        if (inside) dpd = dz.image[pix];
    float T = T_final, last_alpha = 0.0f;
    float accum[3] = {0.0f, 0.0f, 0.0f}, last_col[3] = {0.0f, 0.0f, 0.0f};
    for (int base = 0; base < n; base += kBwdBatch) {   // back to front: entry n-1-base-j
        const int m = min(kBwdBatch, n - base);
        __syncthreads();
        if (tid < m) {
            const unsigned p = ws.vals_out[range.x + (n - 1 - base - tid)];
            const size_t gi = (size_t)v * G + ws.gid[p];
            s_pos[tid] = p;
            s_xy[tid] = ws.xy[gi];
            s_con[tid] = ws.conop[gi];
            if constexpr (COL) {
                s_rgb[tid * 3 + 0] = ws.rgb[gi * 3 + 0];
                s_rgb[tid * 3 + 1] = ws.rgb[gi * 3 + 1];
                s_rgb[tid * 3 + 2] = ws.rgb[gi * 3 + 2];
            }
            if constexpr (DEP) s_d[tid] = dz.values[gi];
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            float val[NS] = {};
            bool hit = false;
            if (n - 1 - base - j < last) {
                const float2 xy = s_xy[j];
                const float4 co = s_con[j];
                const float dx = xy.x - fx, dy = xy.y - fy;
                const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
                if (!(power > 0.0f)) {
                    const float Gs = expf(power);
                    const float alpha = splat_alpha(co.w, Gs);
                    if (!(alpha < 1.0f / 255.0f)) {
                        hit = true;
                        T = T / (1.0f - alpha);
                        const float dchannel = alpha * T;
                        float dL_dalpha = 0.0f;
                        if constexpr (COL)
                            for (int ch = 0; ch < 3; ++ch) {
                                const float c = s_rgb[j * 3 + ch];
                                accum[ch] = last_alpha * last_col[ch] + (1.0f - last_alpha) * accum[ch];
                                last_col[ch] = c;
                                dL_dalpha += (c - accum[ch]) * dp[ch];
                                val[6 + ch] = dchannel * dp[ch];
                            }
                        if constexpr (DEP) {   // the fourth channel; its background is 0
                            const float d = s_d[j];
                            accum_d = last_alpha * last_d + (1.0f - last_alpha) * accum_d;
                            last_d = d;
                            dL_dalpha += (d - accum_d) * dpd;
                            val[NS - 1] = dchannel * dpd;
                        }
                        dL_dalpha *= T;
                        last_alpha = alpha;
                        if constexpr (COL) dL_dalpha += (-T_final / (1.0f - alpha)) * bg_dot;
                        // the 0.99 cap passes the gradient through
                        const float dL_dG = co.w * dL_dalpha;
                        const float gdx = Gs * dx, gdy = Gs * dy;
                        val[0] = dL_dG * (-gdx * co.x - gdy * co.y);   // d / d mean2D, in pixels
                        val[1] = dL_dG * (-gdy * co.z - gdx * co.y);
                        val[2] = -0.5f * gdx * dx * dL_dG;             // d / d conic A, B, C
                        val[3] = -gdx * dy * dL_dG;
                        val[4] = -0.5f * gdy * dy * dL_dG;
                        val[5] = Gs * dL_dalpha;                       // d / d opacity
                    }
                }
            }
            if (__ballot(hit) != 0ull) {
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    if (!splat_slot_used<COL>(k)) continue;
                    const float s = wave_sum_all(val[k]);
                    if (lane == 0) s_part[wave][j][k] = s;
                }
            } else if (lane < NS) {
                s_part[wave][j][lane] = 0.0f;
            }
        }
        __syncthreads();
        for (int e = tid; e < m * NS; e += kThreads) {
            const int j = e / NS, k = e - j * NS;
            if (!splat_slot_used<COL>(k)) continue;
            float s = s_part[0][j][k];
            for (int w = 1; w < kThreads / kWave; ++w) s += s_part[w][j][k];
            slots[(size_t)s_pos[j] * NS + k] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ preprocess backward
// DEP: the tenth slot is added in the same tile-then-view order and chained as dL/dd * d'(z) * dz/dmean, dz/dmean being the third column
// of the view rotation (the scale does not touch it); the term joins the means' gradient after the existing ones.  Without COL no
// harmonics are read and g_sh is not written.
template <bool COL, bool DEP>
__global__ __launch_bounds__(kThreads) void splat_preprocess_bwd_kernel(SplatIn in, const float* __restrict__ cams, SplatWs ws,
                                                                        const float* __restrict__ slots, float* __restrict__ g_means,
                                                                        float* __restrict__ g_cov, float* __restrict__ g_sh,
                                                                        float* __restrict__ g_opac, int V, int G, int d_sh, int use_sh, int H,
                                                                        int W, int K, SplatDepth<DEP> dz) {
    constexpr int NS = DEP ? kSlotDepth : kSlot;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    float gm[3] = {0.0f, 0.0f, 0.0f}, gc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, gop = 0.0f;
    float* gsh = COL ? g_sh + (size_t)g * 3 * d_sh : nullptr;
    if constexpr (COL)
        for (int e = 0; e < 3 * d_sh; ++e) gsh[e] = 0.0f;
    for (int v = 0; v < V; ++v) {
        const size_t i = (size_t)v * G + g;
        const float* cam = cams + (int64_t)v * kCam;
        if (ws.status[v].z) {   // the view did not fit its key capacity: its share of every gradient is NaN
            const float nan = __builtin_nanf("");
            for (int k = 0; k < 3; ++k) gm[k] += nan;
            for (int k = 0; k < 6; ++k) gc[k] += nan;
            gop += nan;
            if constexpr (COL)
                for (int e = 0; e < 3 * d_sh; ++e) gsh[e] += nan;
            continue;
        }
        const unsigned n = ws.touched[i];
        if (n == 0u) continue;
        Geo q;
        if (!splat_project(cam, in, g, H, W, q)) continue;
        // the entries' slots in tile order
        float sl[NS] = {};
        const float* sp = slots + ((size_t)v * K + ws.offs[i]) * NS;
        for (unsigned e = 0; e < n; ++e)
            for (int k = 0; k < NS; ++k)
                if (splat_slot_used<COL>(k)) sl[k] += sp[(size_t)e * NS + k];
        const float s = cam[37], s2 = s * s;
        float dm[3] = {0.0f, 0.0f, 0.0f};   // d / d (mean * scale)
        gop += sl[5];
        // colour
        if constexpr (!COL) {
            // depth alone: nothing to chain
        } else if (use_sh) {
            float nrm[3], len;
            splat_direction(cam, q.m, nrm, len);
            Dual3 basis[kShMax];
            sh_basis<Dual3>(Dual3{nrm[0], 1.0f, 0.0f, 0.0f}, Dual3{nrm[1], 0.0f, 1.0f, 0.0f}, Dual3{nrm[2], 0.0f, 0.0f, 1.0f}, d_sh, basis);
            float gn[3] = {0.0f, 0.0f, 0.0f};
            for (int ch = 0; ch < 3; ++ch) {
                const float* sh = in.sh + g * in.s_g + ch * in.s_ch;
                float acc = 0.0f, ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
#pragma unroll
                for (int k = 0; k < kShMax; ++k)
                    if (k < d_sh) {
                        const float c = sh[k * in.s_k];
                        acc += basis[k].v * c;
                        ddx += basis[k].dx * c;
                        ddy += basis[k].dy * c;
                        ddz += basis[k].dz * c;
                    }
                acc += 0.5f;
                if (acc < 0.0f) continue;   // clamped at 0: no gradient
                const float gcol = sl[6 + ch];
#pragma unroll
                for (int k = 0; k < kShMax; ++k)
                    if (k < d_sh) gsh[ch * d_sh + k] += basis[k].v * gcol;
                gn[0] += ddx * gcol;
                gn[1] += ddy * gcol;
                gn[2] += ddz * gcol;
            }
            const float dot = nrm[0] * gn[0] + nrm[1] * gn[1] + nrm[2] * gn[2];
            for (int k = 0; k < 3; ++k) dm[k] += (gn[k] - nrm[k] * dot) / len;
        } else {
            for (int ch = 0; ch < 3; ++ch) gsh[ch] += sl[6 + ch];
        }
        // conic -> 2-D covariance
        const float a = q.a, b = q.b, c = q.c, det = q.det, inv2 = 1.0f / (det * det);
        const float gA = sl[2], gB = sl[3], gC = sl[4];
        const float ga = (-c * c * gA + b * c * gB - b * b * gC) * inv2;
        const float gb = (2.0f * b * c * gA - (det + 2.0f * b * b) * gB + 2.0f * a * b * gC) * inv2;
        const float gcc = (-b * b * gA + a * b * gB - a * a * gC) * inv2;
        // 2-D covariance -> Sigma (upper triangle, off-diagonals with both symmetric terms) and -> the rows of J R
        const float* M0 = q.M0;
        const float* M1 = q.M1;
        const int ti[6] = {0, 0, 0, 1, 1, 2}, tj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int r = ti[k], cc = tj[k];
            float t = ga * M0[r] * M0[cc] + gcc * M1[r] * M1[cc];
            if (r == cc) t += gb * M0[r] * M1[r];
            else t = 2.0f * t + gb * (M0[r] * M1[cc] + M0[cc] * M1[r]);
            gc[k] += t * s2;
        }
        float gM0[3], gM1[3];
        for (int k = 0; k < 3; ++k) {
            gM0[k] = 2.0f * ga * q.SM0[k] + gb * q.SM1[k];
            gM1[k] = 2.0f * gcc * q.SM1[k] + gb * q.SM0[k];
        }
        // M[a][i] = sum_j J[a][j] view[i][j]
        float gJ00 = 0.0f, gJ02 = 0.0f, gJ11 = 0.0f, gJ12 = 0.0f;
        for (int k = 0; k < 3; ++k) {
            gJ00 += gM0[k] * cam[k * 4 + 0];
            gJ02 += gM0[k] * cam[k * 4 + 2];
            gJ11 += gM1[k] * cam[k * 4 + 1];
            gJ12 += gM1[k] * cam[k * 4 + 2];
        }
        const float tanx = cam[32], tany = cam[33];
        const float fx = (float)W / (2.0f * tanx), fy = (float)H / (2.0f * tany);
        const float tz = q.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
        float gt[3];
        // J02 = -fx tx / tz^2 (free axis) or -fx L / tz with the clamp L = txc / tz (clamped axis: no gradient to tx)
        gt[0] = q.clx ? 0.0f : -fx / tz2 * gJ02;
        gt[1] = q.cly ? 0.0f : -fy / tz2 * gJ12;
        gt[2] = -fx / tz2 * gJ00 - fy / tz2 * gJ11 + (q.clx ? 1.0f : 2.0f) * fx * q.txc / tz3 * gJ02 +
                (q.cly ? 1.0f : 2.0f) * fy * q.tyc / tz3 * gJ12;
        for (int k = 0; k < 3; ++k) dm[k] += gt[0] * cam[k * 4 + 0] + gt[1] * cam[k * 4 + 1] + gt[2] * cam[k * 4 + 2];
        // mean2D -> the homogeneous point (with the 1e-7 of p_w)
        const float gpx = sl[0] * 0.5f * (float)W, gpy = sl[1] * 0.5f * (float)H;
        const float ghx = gpx * q.pw, ghy = gpy * q.pw, ghw = -(gpx * q.hx + gpy * q.hy) * q.pw * q.pw;
        const float* P = cam + 16;
        for (int k = 0; k < 3; ++k) dm[k] += ghx * P[k * 4 + 0] + ghy * P[k * 4 + 1] + ghw * P[k * 4 + 3];
        for (int k = 0; k < 3; ++k) gm[k] += dm[k] * s;
        if constexpr (DEP) {
            const float slope = sl[NS - 1] * splat_depth_slope(dz.mode, q.t[2] / s, dz.near[v], dz.far[v]);
            for (int k = 0; k < 3; ++k) gm[k] += slope * cam[k * 4 + 2];
        }
    }
    for (int k = 0; k < 3; ++k) g_means[(size_t)g * 3 + k] = gm[k];
    float* oc = g_cov + (size_t)g * 9;
    oc[0] = gc[0];
    oc[1] = gc[1];
    oc[2] = gc[2];
    oc[3] = 0.0f;
    oc[4] = gc[3];
    oc[5] = gc[4];
    oc[6] = 0.0f;
    oc[7] = 0.0f;
    oc[8] = gc[5];
    g_opac[g] = gop;
}

// The one argument check of both entry points.  with_depth chooses the slot record the limit counts, 9 or 10 floats per key.
int check_splat(const char* name, int V, int G, int d_sh, int use_sh, int with_depth, int mode, int H, int W, int max_keys) {
    MVS_REQUIRE(V > 0 && G > 0 && H > 0 && W > 0 && max_keys > 0, "%s: bad sizes V=%d G=%d H=%d W=%d max_keys=%d", name, V, G, H, W, max_keys);
    MVS_REQUIRE(d_sh == 1 || d_sh == 4 || d_sh == 9 || d_sh == 16 || d_sh == 25, "%s: d_sh=%d must be 1, 4, 9, 16 or 25", name, d_sh);
    MVS_REQUIRE(use_sh || d_sh == 1, "%s: precomputed colours come as d_sh = 1", name);
    const long long tiles = (long long)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    const int slot = with_depth ? kSlotDepth : kSlot;
    MVS_REQUIRE(V <= 65535 && (long long)V * G < (1ll << 31) && (long long)V * tiles < (1ll << 31) &&
                    (long long)V * max_keys * slot < (1ll << 31) && (long long)V * 3 * H * W < (1ll << 31) && (long long)G * 3 * d_sh < (1ll << 31),
                "%s: V=%d G=%d %dx%d max_keys=%d exceeds the limits (V G, V tiles, %d V max_keys, 3 V H W < 2^31)", name, V, G, H, W, max_keys,
                slot);
    MVS_REQUIRE(!with_depth || (mode >= kModeDepth && mode <= kModeLog),
                "%s: mode=%d must be 0 (depth), 1 (disparity), 2 (relative_disparity) or 3 (log)", name, mode);
    return MVSDET_OK;
}

// The Gaussians as the kernels read them; without colour no harmonics are read and their strides are 0.
SplatIn splat_inputs(const float* means, const int64_t* ms, const float* cov, const int64_t* cs, const float* sh, const int64_t* ss,
                     const float* opac, int64_t os, int with_colour) {
    if (!with_colour) return SplatIn{means, ms[0], ms[1], cov, cs[0], cs[1], cs[2], nullptr, 0, 0, 0, opac, os};
    return SplatIn{means, ms[0], ms[1], cov, cs[0], cs[1], cs[2], sh, ss[0], ss[1], ss[2], opac, os};
}

// The forward launch sequence of every form.  The caller has checked the arguments.
template <bool COL, bool DEP>
int splat_forward(const char* name, const SplatIn& in, const float* cams, const float* background, float* image, void* workspace,
                  size_t workspace_bytes, int V, int G, int d_sh, int use_sh, int H, int W, int max_keys, SplatDepth<DEP> dz, hipStream_t st) {
    MVS_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    const SplatWs ws = splat_layout(workspace, V, G, H, W, max_keys);
    MVS_REQUIRE_WORKSPACE(name, workspace_bytes, ws.total);
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile, tiles = tiles_x * tiles_y;
    const int64_t vg = (int64_t)V * G, vk = (int64_t)V * max_keys;
    hipLaunchKernelGGL((splat_preprocess_kernel<COL, DEP>), dim3((unsigned)((vg + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, in, cams,
                       ws, V, G, d_sh, use_sh, H, W, tiles_x, tiles_y, dz);
    hipLaunchKernelGGL(splat_scan_kernel, dim3(V), dim3(kThreads), 0, st, ws, G, max_keys);
    const int64_t most = vg > vk ? vg : vk;
    const unsigned emit_blocks = (unsigned)((most + kThreads - 1) / kThreads < 4096 ? (most + kThreads - 1) / kThreads : 4096);
    hipLaunchKernelGGL(splat_emit_kernel, dim3(emit_blocks), dim3(kThreads), 0, st, ws, V, G, max_keys, tiles_x, tiles);
    MVS_LAUNCH_CHECK(name);
    const unsigned bits = tile_bits(V, (size_t)tiles);
    size_t sort_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, ws.keys_in, ws.keys_out, ws.vals_in, ws.vals_out, (size_t)vk, 0, 32 + bits, st);
    if (e != hipSuccess || sort_bytes > ws.sort_bytes) {
        set_error("%s: the sort asks for %zu bytes, %zu set aside (%s)", name, sort_bytes, ws.sort_bytes, hipGetErrorString(e));
        return MVSDET_ERR_WORKSPACE;
    }
    sort_bytes = ws.sort_bytes;
    e = rocprim::radix_sort_pairs(ws.sort_tmp, sort_bytes, ws.keys_in, ws.keys_out, ws.vals_in, ws.vals_out, (size_t)vk, 0,
                                                   32 + bits, st);
    if (e != hipSuccess) {
        set_error("%s: sort failed: %s", name, hipGetErrorString(e));
        return MVSDET_ERR_HIP;
    }
    if (hipMemsetAsync(ws.ranges, 0, (size_t)V * tiles * sizeof(int2), st) != hipSuccess) {
        set_error("%s: clearing the tile ranges failed", name);
        return MVSDET_ERR_HIP;
    }
    hipLaunchKernelGGL(splat_ranges_kernel, dim3((unsigned)((vk + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws, vk,
                       (unsigned)(V * tiles));
    hipLaunchKernelGGL((splat_render_kernel<COL, DEP>), dim3(tiles_x, tiles_y, V), dim3(kThreads), 0, st, ws, background, image, G, H, W,
                       tiles_x, tiles, dz);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

// The two launches of every form's backward.
template <bool COL, bool DEP>
int splat_backward(const char* name, const SplatIn& in, const float* cams, const float* background, const float* g_image, void* workspace,
                   size_t workspace_bytes, float* slots, float* g_means, float* g_covariances, float* g_harmonics, float* g_opacities, int V,
                   int G, int d_sh, int use_sh, int H, int W, int max_keys, SplatDepth<DEP> dz, hipStream_t st) {
    MVS_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", name);
    const SplatWs ws = splat_layout(workspace, V, G, H, W, max_keys);
    MVS_REQUIRE_WORKSPACE(name, workspace_bytes, ws.total);
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile, tiles = tiles_x * tiles_y;
    hipLaunchKernelGGL((splat_render_bwd_kernel<COL, DEP>), dim3(tiles_x, tiles_y, V), dim3(kThreads), 0, st, ws, background, g_image, slots,
                       G, H, W, tiles_x, tiles, dz);
    hipLaunchKernelGGL((splat_preprocess_bwd_kernel<COL, DEP>), dim3((G + kWave - 1) / kWave), dim3(kWave), 0, st, in, cams, ws, slots,
                       g_means, g_covariances, g_harmonics, g_opacities, V, G, d_sh, use_sh, H, W, max_keys, dz);
    MVS_LAUNCH_CHECK(name);
    return MVSDET_OK;
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" size_t mvsdet_splat_workspace_bytes(int V, int G, int H, int W, int max_keys) {
    if (check_splat("splat_workspace_bytes", V, G, 1, 1, 0, 0, H, W, max_keys)) return 0;
    return splat_layout(nullptr, V, G, H, W, max_keys).total;
}

extern "C" int mvsdet_splat_cameras_f32(const float* extrinsics, int64_t ext_view_stride, const float* intrinsics, int64_t k_view_stride,
                                        int64_t k_row_stride, const float* near, const float* far, int scale_invariant, float* cams, int V,
                                        mvsdet_stream_t stream) {
    MVS_REQUIRE(extrinsics && intrinsics && near && far && cams, "splat_cameras: NULL pointer");
    MVS_REQUIRE(V > 0 && k_row_stride >= 3, "splat_cameras: bad sizes V=%d, intrinsics rows of %lld elements", V, (long long)k_row_stride);
    hipLaunchKernelGGL(splat_cameras_kernel, dim3((V + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, extrinsics, ext_view_stride,
                       intrinsics, k_view_stride, k_row_stride, near, far, scale_invariant, cams, V);
    MVS_LAUNCH_CHECK("splat_cameras");
    return MVSDET_OK;
}

// with_colour and with_depth choose the form: colour alone <true, false>, colour + depth <true, true>, depth alone <false, true>.
// Without colour harmonics, sh_strides, background and image / g_image / g_harmonics are not read and may be NULL, d_sh and use_sh are
// ignored; without depth the same holds for near, far, depth / g_depth and values, and mode is ignored.
extern "C" int mvsdet_splat_forward_f32(const float* means, const int64_t* means_strides, const float* covariances, const int64_t* cov_strides,
                                        const float* harmonics, const int64_t* sh_strides, const float* opacities, int64_t opacity_stride,
                                        const float* cams, const float* near, const float* far, const float* background, float* image,
                                        float* depth, float* values, void* workspace, size_t workspace_bytes, int V, int G, int d_sh,
                                        int use_sh, int with_colour, int with_depth, int mode, int H, int W, int max_keys,
                                        mvsdet_stream_t stream) {
    const char* name = "splat_forward";
    MVS_REQUIRE(with_colour || with_depth, "%s: neither colour nor depth is asked for (with_colour = with_depth = 0)", name);
    if (!with_colour) d_sh = 1, use_sh = 0;
    if (int rc = check_splat(name, V, G, d_sh, use_sh, with_depth, mode, H, W, max_keys)) return rc;
    MVS_REQUIRE(means && means_strides && covariances && cov_strides && opacities && cams && workspace &&
                    (!with_colour || (harmonics && sh_strides && background && image)) && (!with_depth || (near && far && depth && values)),
                "%s: NULL pointer", name);
    const SplatIn in = splat_inputs(means, means_strides, covariances, cov_strides, harmonics, sh_strides, opacities, opacity_stride, with_colour);
    const SplatDepth<true> dz{near, far, values, depth, mode};
    const hipStream_t st = (hipStream_t)stream;
    if (!with_depth)
        return splat_forward<true, false>(name, in, cams, background, image, workspace, workspace_bytes, V, G, d_sh, use_sh, H, W, max_keys,
                                          SplatDepth<false>{}, st);
    if (with_colour)
        return splat_forward<true, true>(name, in, cams, background, image, workspace, workspace_bytes, V, G, d_sh, use_sh, H, W, max_keys, dz,
                                         st);
    return splat_forward<false, true>(name, in, cams, nullptr, nullptr, workspace, workspace_bytes, V, G, d_sh, use_sh, H, W, max_keys, dz, st);
}

extern "C" int mvsdet_splat_backward_f32(const float* means, const int64_t* means_strides, const float* covariances, const int64_t* cov_strides,
                                         const float* harmonics, const int64_t* sh_strides, const float* opacities, int64_t opacity_stride,
                                         const float* cams, const float* near, const float* far, const float* background,
                                         const float* g_image, const float* g_depth, const float* values, void* workspace,
                                         size_t workspace_bytes, float* slots, float* g_means, float* g_covariances, float* g_harmonics,
                                         float* g_opacities, int V, int G, int d_sh, int use_sh, int with_colour, int with_depth, int mode,
                                         int H, int W, int max_keys, mvsdet_stream_t stream) {
    const char* name = "splat_backward";
    MVS_REQUIRE(with_colour || with_depth, "%s: neither colour nor depth is asked for (with_colour = with_depth = 0)", name);
    if (!with_colour) d_sh = 1, use_sh = 0;
    if (int rc = check_splat(name, V, G, d_sh, use_sh, with_depth, mode, H, W, max_keys)) return rc;
    MVS_REQUIRE(means && means_strides && covariances && cov_strides && opacities && cams && workspace && slots && g_means && g_covariances &&
                    g_opacities && (!with_colour || (harmonics && sh_strides && background && g_image && g_harmonics)) &&
                    (!with_depth || (near && far && g_depth && values)),
                "%s: NULL pointer", name);
    const SplatIn in = splat_inputs(means, means_strides, covariances, cov_strides, harmonics, sh_strides, opacities, opacity_stride, with_colour);
    // the kernels only read values and g_depth; the struct is shared with the forward, which writes them
    const SplatDepth<true> dz{near, far, const_cast<float*>(values), const_cast<float*>(g_depth), mode};
    const hipStream_t st = (hipStream_t)stream;
    if (!with_depth)
        return splat_backward<true, false>(name, in, cams, background, g_image, workspace, workspace_bytes, slots, g_means, g_covariances,
                                           g_harmonics, g_opacities, V, G, d_sh, use_sh, H, W, max_keys, SplatDepth<false>{}, st);
    if (with_colour)
        return splat_backward<true, true>(name, in, cams, background, g_image, workspace, workspace_bytes, slots, g_means, g_covariances,
                                          g_harmonics, g_opacities, V, G, d_sh, use_sh, H, W, max_keys, dz, st);
    return splat_backward<false, true>(name, in, cams, nullptr, nullptr, workspace, workspace_bytes, slots, g_means, g_covariances, nullptr,
                                       g_opacities, V, G, d_sh, use_sh, H, W, max_keys, dz, st);
}
