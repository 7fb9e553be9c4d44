// Photometric consistency on gfx950: the reference's self-supervised depth objective and its gradients.
//   inverse_warping / _bilinear_sample / compute_reconstr_loss (mvs_models/homography.py), MVSDet.photometric_loss (mvsdet.py:845-874).
// Geometry (one launch, one thread per (chosen view, its source view) pair): K_left^-1 and K_left [R_rel | t_rel] in float64 from the
// fp32 cameras, rounded ONCE to fp32 -- no torch.inverse, no host synchronisation.  The LEFT intrinsics project into the right view, as
// the reference has it.
// Warp (one launch, one thread per (b, y, x), lanes along x): the reference's fp32 operation order from the linspace pixel grid (two
// short vectors from the host) through z + 1e-10, the normalise / denormalise round trip, floor, the mask (x0 >= 0, x1 <= W-1, y0 >= 0,
// y0 <= H-1: on y0), the four clamped taps and the weights formed from the CLAMPED x1, y1.  Depth and image are read in place through
// strides and index vectors.
// Loss (two launches): fp32 terms of the three smooth-L1 sums added in float64 per wave, per block, over the blocks in the one fixed
// order of block_reduce.h.
// Selection over scenes (two launches): per pixel the scene of the smallest L_i + 1e4 (1 - mask_i), ties to the lower index.
// Backward: one launch each for the loss (d L / d warped, pixel-centric: photo term and the transposed difference stencils, times the
// mask) and for the warp (through the four weights to (x, y), through the quotient to depth).  No atomics anywhere.
//
// Roofline: neither.  B*h*w = 47 200 pixels per scene: the launches bound it.
#include "block_reduce.h"
#include "camera_math.h"

namespace mvsdet {

constexpr int kPhotoGeo = 24;        // floats per pair: K^-1 (9, row-major), K [R_rel | t_rel] (12, row-major 3x4), 3 unused
constexpr int kPhotoMaxScenes = 32;  // photometric_select: scenes per call

struct PhotoPartial {
    double s0, s1, s2;   // photo, d/dx, d/dy smooth-L1 sums
    long long n;         // pixels inside the mask
    __device__ void add(const PhotoPartial& r) {
        s0 = s0 + r.s0;
        s1 = s1 + r.s1;
        s2 = s2 + r.s2;
        n += r.n;
    }
};

// ---------------------------------------------------------------------------------------------------------------- geometry
// ext: (.,r>=3,4) rows of [R|t]; K: rows of the intrinsics; strides in elements.  idx NULL = the pair's own number.
__global__ void photo_geometry_kernel(const float* __restrict__ ext_l, int64_t el_view, const float* __restrict__ k_l, int64_t kl_view,
                                      int64_t k_row, const float* __restrict__ ext_r, int64_t er_view, const int64_t* __restrict__ l_idx,
                                      const int64_t* __restrict__ r_idx, int n_left, int n_right, float* __restrict__ geo, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* g = geo + (int64_t)b * kPhotoGeo;
    const int64_t li = l_idx ? l_idx[b] : b, ri = r_idx ? r_idx[b] : b;
    if (li < 0 || li >= n_left || ri < 0 || ri >= n_right) {   // an index outside the views: NaN geometry, nothing is read
        for (int i = 0; i < kPhotoGeo; ++i) g[i] = __builtin_nanf("");
        return;
    }
    const float* L = ext_l + li * el_view;
    const float* R = ext_r + ri * er_view;
    const float* Kp = k_l + li * kl_view;
    double K[3][3], Rl[3][3], Rr[3][3], tl[3], tr[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            K[i][j] = (double)Kp[i * k_row + j];
            Rl[i][j] = (double)L[i * 4 + j];
            Rr[i][j] = (double)R[i * 4 + j];
        }
        tl[i] = (double)L[i * 4 + 3];
        tr[i] = (double)R[i * 4 + 3];
    }
    // adjugate / determinant
    double inv[3][3];
    inverse3(K, inv);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) g[i * 3 + j] = (float)inv[i][j];
    // T = [R_r R_l^T | t_r - R_rel t_l], P = K T
    double T[3][4];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[i][j] = Rr[i][0] * Rl[j][0] + Rr[i][1] * Rl[j][1] + Rr[i][2] * Rl[j][2];
        T[i][3] = tr[i] - (T[i][0] * tl[0] + T[i][1] * tl[1] + T[i][2] * tl[2]);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) g[9 + i * 4 + j] = (float)(K[i][0] * T[0][j] + K[i][1] * T[1][j] + K[i][2] * T[2][j]);
    g[21] = g[22] = g[23] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------- warp
struct PhotoTaps {
    int x0, x1, y0, y1;   // clamped
    float ax, ay;         // clamped x1 - x, clamped y1 - y
    bool in;
    float r0, r1, r2;     // K^-1 [xg, yg, 1]
    float p0, p1, z;      // projected point, z = p2 + 1e-10
};

// homography.py:86-101, 109-113, 146-162, 192-195 in fp32, in the reference's order.
__device__ __forceinline__ PhotoTaps photo_taps(const float* __restrict__ g, float xg, float yg, float depth, int h, int w) {
    PhotoTaps t;
    t.r0 = g[0] * xg + g[1] * yg + g[2];
    t.r1 = g[3] * xg + g[4] * yg + g[5];
    t.r2 = g[6] * xg + g[7] * yg + g[8];
    const float c0 = t.r0 * depth, c1 = t.r1 * depth, c2 = t.r2 * depth;
    t.p0 = g[9] * c0 + g[10] * c1 + g[11] * c2 + g[12];
    t.p1 = g[13] * c0 + g[14] * c1 + g[15] * c2 + g[16];
    const float p2 = g[17] * c0 + g[18] * c1 + g[19] * c2 + g[20];
    t.z = p2 + 1e-10f;
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const float nx = t.p0 / t.z / wm1 * 2.0f - 1.0f, ny = t.p1 / t.z / hm1 * 2.0f - 1.0f;
    const float x = (nx + 1.0f) * wm1 / 2.0f, y = (ny + 1.0f) * hm1 / 2.0f;
    const float fx = floorf(x), fy = floorf(y);
    t.in = (fx >= 0.0f) && (fx + 1.0f <= wm1) && (fy >= 0.0f) && (fy <= hm1);   // NaN stays outside
    // clamped in float first: no integer overflow for far-away positions; NaN lands on index 0
    const float x0c = fminf(fmaxf(fx, 0.0f), wm1), x1c = fminf(fmaxf(fx + 1.0f, 0.0f), wm1);
    const float y0c = fminf(fmaxf(fy, 0.0f), hm1), y1c = fminf(fmaxf(fy + 1.0f, 0.0f), hm1);
    t.x0 = clampi((int)x0c, 0, w - 1);
    t.x1 = clampi((int)x1c, 0, w - 1);
    t.y0 = clampi((int)y0c, 0, h - 1);
    t.y1 = clampi((int)y1c, 0, h - 1);
    t.ax = x1c - x;
    t.ay = y1c - y;
    return t;
}

struct PhotoImage {
    const float* p;
    int64_t s0, s1, s2, s3;   // view, y, x, channel
};

__global__ __launch_bounds__(kThreads) void photo_warp_kernel(PhotoImage img, const int64_t* __restrict__ src_idx, int n_img,
                                                              const float* __restrict__ depth, int64_t ds0, int64_t ds1, int64_t ds2,
                                                              const int64_t* __restrict__ depth_idx, int n_depth,
                                                              const float* __restrict__ geo, const float* __restrict__ xg,
                                                              const float* __restrict__ yg, float* __restrict__ warped,
                                                              float* __restrict__ mask, int total, int h, int w, int C) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= total) return;
    const int hw = h * w;
    const int b = p / hw, r = p - b * hw;
    const int y = r / w, x = r - y * w;
    const int64_t si = src_idx ? src_idx[b] : b, di = depth_idx ? depth_idx[b] : b;
    float* out = warped + (int64_t)p * C;
    if (si < 0 || si >= n_img || di < 0 || di >= n_depth) {   // an index outside the views: NaN, outside the mask, nothing is read
        for (int c = 0; c < C; ++c) out[c] = __builtin_nanf("");
        mask[p] = 0.0f;
        return;
    }
    const float d = depth[di * ds0 + (int64_t)y * ds1 + (int64_t)x * ds2];
    const PhotoTaps t = photo_taps(geo + (int64_t)b * kPhotoGeo, xg[x], yg[y], d, h, w);
    const float by = 1.0f - t.ay, bx = 1.0f - t.ax;
    const float wa = t.ax * t.ay, wb = t.ax * by, wc = bx * t.ay, wd = bx * by;
    const float* base = img.p + si * img.s0;
    const float* pa = base + t.y0 * img.s1 + t.x0 * img.s2;
    const float* pb = base + t.y1 * img.s1 + t.x0 * img.s2;
    const float* pc = base + t.y0 * img.s1 + t.x1 * img.s2;
    const float* pd = base + t.y1 * img.s1 + t.x1 * img.s2;
    for (int c = 0; c < C; ++c) {
        const int64_t o = c * img.s3;
        out[c] = wa * pa[o] + wb * pb[o] + wc * pc[o] + wd * pd[o];
    }
    mask[p] = t.in ? 1.0f : 0.0f;
}

// d warped / d depth, summed over the pairs b that read depth view n (in ascending b): grad (Nd,h,w) dense.
// A pixel whose incoming gradient is 0 in every channel contributes exactly 0 whatever its position (Inf, NaN).
__global__ __launch_bounds__(kThreads) void photo_warp_bwd_kernel(PhotoImage img, const int64_t* __restrict__ src_idx, int n_img,
                                                                  const float* __restrict__ depth, int64_t ds0, int64_t ds1,
                                                                  int64_t ds2, const int64_t* __restrict__ depth_idx, int n_depth,
                                                                  const float* __restrict__ geo, const float* __restrict__ xg,
                                                                  const float* __restrict__ yg, const float* __restrict__ g_warped,
                                                                  float* __restrict__ grad, int total, int B, int h, int w, int C) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= total) return;   // total = n_depth * h * w
    const int hw = h * w;
    const int n = p / hw, r = p - n * hw;
    const int y = r / w, x = r - y * w;
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) {
        const int64_t di = depth_idx ? depth_idx[b] : b;
        if (di != n) continue;
        const int64_t si = src_idx ? src_idx[b] : b;
        if (si < 0 || si >= n_img) continue;
        const float* g = g_warped + ((int64_t)b * hw + r) * C;
        bool any = false;
        for (int c = 0; c < C; ++c) any = any || (g[c] != 0.0f);
        if (!any) continue;
        const float d = depth[(int64_t)n * ds0 + (int64_t)y * ds1 + (int64_t)x * ds2];
        const float* G = geo + (int64_t)b * kPhotoGeo;
        const PhotoTaps t = photo_taps(G, xg[x], yg[y], d, h, w);
        const float by = 1.0f - t.ay, bx = 1.0f - t.ax;
        const float* base = img.p + si * img.s0;
        const float* pa = base + t.y0 * img.s1 + t.x0 * img.s2;
        const float* pb = base + t.y1 * img.s1 + t.x0 * img.s2;
        const float* pc = base + t.y0 * img.s1 + t.x1 * img.s2;
        const float* pd = base + t.y1 * img.s1 + t.x1 * img.s2;
        float gx = 0.0f, gy = 0.0f;   // d / d x, d / d y: the weights are (x1 - x)(y1 - y), ... with x1, y1 constants
        for (int c = 0; c < C; ++c) {
            const int64_t o = c * img.s3;
            const float va = pa[o], vb = pb[o], vc = pc[o], vd = pd[o];
            gx = gx + g[c] * (t.ay * (vc - va) + by * (vd - vb));
            gy = gy + g[c] * (t.ax * (vb - va) + bx * (vd - vc));
        }
        // x = p0 / z, p_i = (P_i . r) depth + P_i3: d x / d depth = (q0 - x q2) / z, the small difference formed in float64
        const double q0 = (double)G[9] * t.r0 + (double)G[10] * t.r1 + (double)G[11] * t.r2;
        const double q1 = (double)G[13] * t.r0 + (double)G[14] * t.r1 + (double)G[15] * t.r2;
        const double q2 = (double)G[17] * t.r0 + (double)G[18] * t.r1 + (double)G[19] * t.r2;
        const double z = (double)t.z;
        const double dx = (q0 - (double)t.p0 / z * q2) / z, dy = (q1 - (double)t.p1 / z * q2) / z;
        acc = acc + (float)((double)gx * dx + (double)gy * dy);
    }
    grad[p] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ float smooth_l1(float d) {
    const float a = fabsf(d);
    return a < 1.0f ? 0.5f * a * a : a - 0.5f;
}
__device__ __forceinline__ float smooth_l1_grad(float d) { return d > 1.0f ? 1.0f : (d < -1.0f ? -1.0f : d); }

// warped (B,h,w,C) contiguous, mask (B,h,w) contiguous, ref through its strides.
__global__ __launch_bounds__(kThreads) void photo_loss_kernel(const float* __restrict__ warped, const float* __restrict__ mask,
                                                              PhotoImage ref, PhotoPartial* __restrict__ part, int total, int h, int w,
                                                              int C, int simple) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    int in_mask = 0;
    if (p < total) {
        const int hw = h * w;
        const int b = p / hw, r = p - b * hw;
        const int y = r / w, x = r - y * w;
        const float m = mask[p];
        in_mask = m != 0.0f;
        const bool has_x = !simple && x + 1 < w, has_y = !simple && y + 1 < h;
        const float mx = has_x ? mask[p + 1] : 0.0f, my = has_y ? mask[p + w] : 0.0f;
        const float* wp = warped + (int64_t)p * C;
        const float* rp = ref.p + b * ref.s0 + y * ref.s1 + x * ref.s2;
        for (int c = 0; c < C; ++c) {
            const float wm = wp[c] * m, rm = rp[c * ref.s3] * m;
            t0 = t0 + smooth_l1(wm - rm);
            if (has_x) t1 = t1 + smooth_l1((wp[C + c] * mx - wm) - (rp[ref.s2 + c * ref.s3] * mx - rm));
            if (has_y) t2 = t2 + smooth_l1((wp[(int64_t)w * C + c] * my - wm) - (rp[ref.s1 + c * ref.s3] * my - rm));
        }
    }
    double a[3] = {(double)t0, (double)t1, (double)t2};
    int n[1] = {in_mask};
    if (block_sums(a, n)) part[blockIdx.x] = {a[0], a[1], a[2], n[0]};
}

// One block; every partial enters in ascending block order (block_reduce.h's ordered_partial_sum).
// loss = L, terms = the three means; an empty difference term (w = 1 or h = 1) is 0 / 0 = NaN as torch.mean of nothing.
__global__ __launch_bounds__(kThreads) void photo_loss_finish_kernel(const PhotoPartial* __restrict__ part, int nblocks,
                                                                     float* __restrict__ loss, float* __restrict__ terms,
                                                                     int32_t* __restrict__ count, double n0, double n1, double n2,
                                                                     int simple) {
    PhotoPartial a;
    if (ordered_partial_sum(part, nblocks, a)) {
        const float m0 = (float)(a.s0 / n0);
        const float m1 = simple ? 0.0f : (float)(a.s1 / n1), m2 = simple ? 0.0f : (float)(a.s2 / n2);
        loss[0] = simple ? m0 : 0.5f * m0 + 0.5f * (m1 + m2);   // (1 - alpha) photo + alpha (dx + dy), alpha = 0.5
        terms[0] = m0;
        terms[1] = m1;
        terms[2] = m2;
        count[0] = (int32_t)a.n;
    }
}

// d L / d warped (B,h,w,C) = mask * d L / d wm: the photo term and the transposed forward differences.
__global__ __launch_bounds__(kThreads) void photo_loss_bwd_kernel(const float* __restrict__ warped, const float* __restrict__ mask,
                                                                  PhotoImage ref, const float* __restrict__ g_loss,
                                                                  float* __restrict__ grad, int total, int h, int w, int C, float k0,
                                                                  float k1, float k2) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= total) return;
    float* out = grad + (int64_t)p * C;
    const float m = mask[p];
    if (m == 0.0f) {
        for (int c = 0; c < C; ++c) out[c] = 0.0f;
        return;
    }
    const int hw = h * w;
    const int b = p / hw, r = p - b * hw;
    const int y = r / w, x = r - y * w;
    const bool simple = k1 == 0.0f && k2 == 0.0f;
    const bool xn = !simple && x + 1 < w, xp = !simple && x > 0, yn = !simple && y + 1 < h, yp = !simple && y > 0;
    const float mxn = xn ? mask[p + 1] : 0.0f, mxp = xp ? mask[p - 1] : 0.0f;
    const float myn = yn ? mask[p + w] : 0.0f, myp = yp ? mask[p - w] : 0.0f;
    const float* wp = warped + (int64_t)p * C;
    const float* rp = ref.p + b * ref.s0 + y * ref.s1 + x * ref.s2;
    const float gl = g_loss[0];
    const int64_t wC = (int64_t)w * C;
    for (int c = 0; c < C; ++c) {
        const int64_t rc = c * ref.s3;
        const float wm = wp[c] * m, rm = rp[rc] * m;
        float g = k0 * smooth_l1_grad(wm - rm);
        float gxs = 0.0f, gys = 0.0f;
        if (xn) gxs = gxs - smooth_l1_grad((wp[C + c] * mxn - wm) - (rp[ref.s2 + rc] * mxn - rm));
        if (xp) gxs = gxs + smooth_l1_grad((wm - wp[c - C] * mxp) - (rm - rp[rc - ref.s2] * mxp));
        if (yn) gys = gys - smooth_l1_grad((wp[wC + c] * myn - wm) - (rp[ref.s1 + rc] * myn - rm));
        if (yp) gys = gys + smooth_l1_grad((wm - wp[c - wC] * myp) - (rm - rp[rc - ref.s1] * myp));
        g = g + k1 * gxs + k2 * gys;
        out[c] = gl * g * m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- selection
// masks (n, total) contiguous, L (n).  Per pixel: v_i = L_i + 1e4 (1 - mask_i); the smallest v (the lower index on a tie) wins the pixel
// if it is < 1e4.  part[block][n] win counts.
__global__ __launch_bounds__(kThreads) void photo_select_kernel(const float* __restrict__ masks, const float* __restrict__ L,
                                                                int32_t* __restrict__ part, int n, int total) {
    __shared__ int s_n[kPhotoMaxScenes][kThreads / kWave];
    const int p = blockIdx.x * kThreads + threadIdx.x;
    int win = -1;
    if (p < total) {
        float best = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float v = L[i] + 1e4f * (1.0f - masks[(int64_t)i * total + p]);
            if (i == 0 || v < best) {
                best = v;
                win = i;
            }
        }
        if (!(best < 1e4f)) win = -1;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int i = 0; i < n; ++i) {
        const int c = wave_sum(win == i ? 1 : 0);
        if (lane == 0) s_n[i][wave] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
        int c = 0;
        for (int k = 0; k < kThreads / kWave; ++k) c += s_n[threadIdx.x][k];
        part[(int64_t)blockIdx.x * n + threadIdx.x] = c;
    }
}

// One block: thread i < n adds scene i's counts over the blocks; thread 0 then forms loss_pc = sum_i wins_i L_i / total in float64.
__global__ __launch_bounds__(kThreads) void photo_select_finish_kernel(const int32_t* __restrict__ part, const float* __restrict__ L,
                                                                       int32_t* __restrict__ wins, float* __restrict__ loss, int n,
                                                                       int nblocks, int total) {
    __shared__ long long s_w[kPhotoMaxScenes];
    if ((int)threadIdx.x < n) {
        long long c = 0;
        for (int b = 0; b < nblocks; ++b) c += part[(int64_t)b * n + threadIdx.x];
        s_w[threadIdx.x] = c;
        wins[threadIdx.x] = (int32_t)c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i)
            if (s_w[i] > 0) s = s + (double)s_w[i] * (double)L[i];
        loss[0] = (float)(s / (double)total);
    }
}

// d loss_pc / d L_i = g wins_i / total
__global__ void photo_select_bwd_kernel(const int32_t* __restrict__ wins, const float* __restrict__ g_loss, float* __restrict__ grad,
                                        int n, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) grad[i] = g_loss[0] * (float)((double)wins[i] / (double)total);
}

}  // namespace mvsdet

using namespace mvsdet;

static int check_photo_shape(const char* name, int B, int h, int w, int C) {
    MVS_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0, "%s: bad shape B=%d h=%d w=%d C=%d", name, B, h, w, C);
    MVS_REQUIRE((long long)B * h * w * C < (long long)INT32_MAX, "%s: %dx%dx%dx%d exceeds 2^31 elements", name, B, h, w, C);
    return MVSDET_OK;
}

extern "C" int mvsdet_photo_geometry_f32(const float* ext_left, int64_t ext_left_view_stride, const float* k_left,
                                         int64_t k_view_stride, int64_t k_row_stride, const float* ext_right,
                                         int64_t ext_right_view_stride, const int64_t* left_idx, const int64_t* right_idx, int n_left,
                                         int n_right, float* geo, int B, mvsdet_stream_t stream) {
    MVS_REQUIRE(ext_left && k_left && ext_right && geo, "photo_geometry: NULL pointer");
    MVS_REQUIRE(B > 0 && n_left > 0 && n_right > 0, "photo_geometry: bad sizes B=%d n_left=%d n_right=%d", B, n_left, n_right);
    MVS_REQUIRE(k_row_stride >= 3, "photo_geometry: intrinsics rows of %lld elements", (long long)k_row_stride);
    hipLaunchKernelGGL(photo_geometry_kernel, dim3((B + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, ext_left,
                       ext_left_view_stride, k_left, k_view_stride, k_row_stride, ext_right, ext_right_view_stride, left_idx, right_idx,
                       n_left, n_right, geo, B);
    MVS_LAUNCH_CHECK("photo_geometry");
    return MVSDET_OK;
}

static int check_photo_warp(const char* name, const float* img, const int64_t* is, const float* depth, const int64_t* ds, const float* geo,
                            const float* xg, const float* yg, int n_img, int n_depth, int B, int h, int w, int C) {
    if (int rc = check_photo_shape(name, B, h, w, C)) return rc;
    MVS_REQUIRE(img && is && depth && ds && geo && xg && yg, "%s: NULL pointer", name);
    MVS_REQUIRE(n_img > 0 && n_depth > 0, "%s: bad view counts %d / %d", name, n_img, n_depth);
    MVS_REQUIRE((long long)n_depth * h * w < (long long)INT32_MAX, "%s: %dx%dx%d exceeds 2^31 pixels", name, n_depth, h, w);
    return MVSDET_OK;
}

extern "C" int mvsdet_photo_warp_f32(const float* img, const int64_t* img_strides, const int64_t* src_idx, int n_img, const float* depth,
                                     const int64_t* depth_strides, const int64_t* depth_idx, int n_depth, const float* geo,
                                     const float* xg, const float* yg, float* warped, float* mask, int B, int h, int w, int C,
                                     mvsdet_stream_t stream) {
    if (int rc = check_photo_warp("photo_warp", img, img_strides, depth, depth_strides, geo, xg, yg, n_img, n_depth, B, h, w, C)) return rc;
    MVS_REQUIRE(warped && mask, "photo_warp: NULL pointer");
    MVS_REQUIRE(src_idx || n_img == B, "photo_warp: %d images for %d pairs and no index", n_img, B);
    MVS_REQUIRE(depth_idx || n_depth == B, "photo_warp: %d depth maps for %d pairs and no index", n_depth, B);
    const PhotoImage im = {img, img_strides[0], img_strides[1], img_strides[2], img_strides[3]};
    const int total = B * h * w;
    hipLaunchKernelGGL(photo_warp_kernel, dim3((int)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, im, src_idx, n_img, depth,
                       depth_strides[0], depth_strides[1], depth_strides[2], depth_idx, n_depth, geo, xg, yg, warped, mask, total, h, w, C);
    MVS_LAUNCH_CHECK("photo_warp");
    return MVSDET_OK;
}

extern "C" int mvsdet_photo_warp_bwd_f32(const float* img, const int64_t* img_strides, const int64_t* src_idx, int n_img,
                                         const float* depth, const int64_t* depth_strides, const int64_t* depth_idx, int n_depth,
                                         const float* geo, const float* xg, const float* yg, const float* g_warped, float* grad, int B,
                                         int h, int w, int C, mvsdet_stream_t stream) {
    if (int rc = check_photo_warp("photo_warp_bwd", img, img_strides, depth, depth_strides, geo, xg, yg, n_img, n_depth, B, h, w, C))
        return rc;
    MVS_REQUIRE(g_warped && grad, "photo_warp_bwd: NULL pointer");
    MVS_REQUIRE(src_idx || n_img == B, "photo_warp_bwd: %d images for %d pairs and no index", n_img, B);
    MVS_REQUIRE(depth_idx || n_depth == B, "photo_warp_bwd: %d depth maps for %d pairs and no index", n_depth, B);
    const PhotoImage im = {img, img_strides[0], img_strides[1], img_strides[2], img_strides[3]};
    const int total = n_depth * h * w;
    hipLaunchKernelGGL(photo_warp_bwd_kernel, dim3((int)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, im, src_idx, n_img, depth,
                       depth_strides[0], depth_strides[1], depth_strides[2], depth_idx, n_depth, geo, xg, yg, g_warped, grad, total, B, h,
                       w, C);
    MVS_LAUNCH_CHECK("photo_warp_bwd");
    return MVSDET_OK;
}

extern "C" size_t mvsdet_photo_loss_workspace_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)blocks_of((long long)B * h * w) * sizeof(PhotoPartial);
}

extern "C" int mvsdet_photo_loss_f32(const float* warped, const float* mask, const float* ref, const int64_t* ref_strides, float* loss,
                                     float* terms, int32_t* count, void* workspace, size_t workspace_bytes, int B, int h, int w, int C, int simple,
                                     mvsdet_stream_t stream) {
    if (int rc = check_photo_shape("photo_loss", B, h, w, C)) return rc;
    MVS_REQUIRE(warped && mask && ref && ref_strides && loss && terms && count && workspace, "photo_loss: NULL pointer");
    MVS_REQUIRE(((uintptr_t)workspace & 15) == 0, "photo_loss: workspace must be 16-byte aligned");
    MVS_REQUIRE_WORKSPACE("photo_loss", workspace_bytes, mvsdet_photo_loss_workspace_bytes(B, h, w));
    const PhotoImage rf = {ref, ref_strides[0], ref_strides[1], ref_strides[2], ref_strides[3]};
    const int total = B * h * w, nblocks = (int)blocks_of(total);
    PhotoPartial* part = (PhotoPartial*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(photo_loss_kernel, dim3(nblocks), dim3(kThreads), 0, st, warped, mask, rf, part, total, h, w, C, simple ? 1 : 0);
    MVS_LAUNCH_CHECK("photo_loss (terms)");
    const double n0 = (double)B * h * w * C, n1 = (double)B * h * (w - 1) * C, n2 = (double)B * (h - 1) * w * C;
    hipLaunchKernelGGL(photo_loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, part, nblocks, loss, terms, count, n0, n1, n2, simple ? 1 : 0);
    MVS_LAUNCH_CHECK("photo_loss (finish)");
    return MVSDET_OK;
}

extern "C" int mvsdet_photo_loss_bwd_f32(const float* warped, const float* mask, const float* ref, const int64_t* ref_strides,
                                         const float* g_loss, float* grad, int B, int h, int w, int C, int simple,
                                         mvsdet_stream_t stream) {
    if (int rc = check_photo_shape("photo_loss_bwd", B, h, w, C)) return rc;
    MVS_REQUIRE(warped && mask && ref && ref_strides && g_loss && grad, "photo_loss_bwd: NULL pointer");
    const PhotoImage rf = {ref, ref_strides[0], ref_strides[1], ref_strides[2], ref_strides[3]};
    const int total = B * h * w;
    const double n0 = (double)B * h * w * C, n1 = (double)B * h * (w - 1) * C, n2 = (double)B * (h - 1) * w * C;
    // the weight of one term in L: (1 - alpha) / n0, alpha / n1, alpha / n2; an empty difference term has no element to weigh
    const float k0 = (float)((simple ? 1.0 : 0.5) / n0);
    const float k1 = (simple || n1 <= 0) ? 0.0f : (float)(0.5 / n1), k2 = (simple || n2 <= 0) ? 0.0f : (float)(0.5 / n2);
    hipLaunchKernelGGL(photo_loss_bwd_kernel, dim3((int)blocks_of(total)), dim3(kThreads), 0, (hipStream_t)stream, warped, mask, rf, g_loss,
                       grad, total, h, w, C, k0, k1, k2);
    MVS_LAUNCH_CHECK("photo_loss_bwd");
    return MVSDET_OK;
}

extern "C" size_t mvsdet_photo_select_workspace_bytes(int n, int total) {
    if (n <= 0 || total <= 0) return 0;
    return (size_t)blocks_of(total) * n * sizeof(int32_t);
}

extern "C" int mvsdet_photo_select_f32(const float* masks, const float* L, int32_t* wins, float* loss, void* workspace,
                                       size_t workspace_bytes, int n, int total, mvsdet_stream_t stream) {
    MVS_REQUIRE(masks && L && wins && loss && workspace, "photo_select: NULL pointer");
    MVS_REQUIRE(n > 0 && n <= kPhotoMaxScenes, "photo_select: %d scenes (1..%d)", n, kPhotoMaxScenes);
    MVS_REQUIRE(total > 0, "photo_select: bad pixel count %d", total);
    MVS_REQUIRE_WORKSPACE("photo_select", workspace_bytes, mvsdet_photo_select_workspace_bytes(n, total));
    const int nblocks = (int)blocks_of(total);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(photo_select_kernel, dim3(nblocks), dim3(kThreads), 0, st, masks, L, (int32_t*)workspace, n, total);
    MVS_LAUNCH_CHECK("photo_select (wins)");
    hipLaunchKernelGGL(photo_select_finish_kernel, dim3(1), dim3(kThreads), 0, st, (const int32_t*)workspace, L, wins, loss, n, nblocks,
                       total);
    MVS_LAUNCH_CHECK("photo_select (finish)");
    return MVSDET_OK;
}

extern "C" int mvsdet_photo_select_bwd_f32(const int32_t* wins, const float* g_loss, float* grad, int n, int total,
                                           mvsdet_stream_t stream) {
    MVS_REQUIRE(wins && g_loss && grad, "photo_select_bwd: NULL pointer");
    MVS_REQUIRE(n > 0 && n <= kPhotoMaxScenes && total > 0, "photo_select_bwd: bad sizes n=%d total=%d", n, total);
    hipLaunchKernelGGL(photo_select_bwd_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, wins, g_loss, grad, n, total);
    MVS_LAUNCH_CHECK("photo_select_bwd");
    return MVSDET_OK;
}
