// Gaussian adapter: the pixel Gaussians that the rasteriser (csrc/splat.hip) renders -- GaussianAdapter.forward
// (gs_src/model/encoder/common/gaussian_adapter.py:50-98) with the offset lines of mvsdet.py:576-578.  DESIGN.md 4.16.
//
//   cameras   one thread per view: C_v, origin, K_v^-1 (adjugate), the scale multiplier m_v and the rotation blocks D_l of the
//             harmonics (built from csrc/sh_basis.h on double against the constant tables of adapter_sh_table.h, or copied from the
//             caller), float64 inside, rounded once
//   forward   one block per 64 consecutive Gaussians of ONE view: the 64 rows of `raw` come in with full-width coalesced loads into
//             LDS (row pitch odd: a lane walking its own row meets no bank conflict); waves 0..2 rotate the harmonics of colour
//             channel 0..2 (the view's D_l are uniform: scalar loads), wave 3 does offset, scales, quaternion, covariance and mean;
//             results go back through LDS and leave with coalesced stores
//   backward  the same shape: the transposed block-diagonal product on waves 0..2, the geometry's chain rule on wave 3; every
//             Gaussian's gradient lands in its own row, so there are no atomics and two runs give the same bits
#include "camera_math.h"
#include "common.h"
#include "sh_basis.h"

namespace mvsdet {
template <>
__host__ __device__ __forceinline__ double sh_one<double>(double) { return 1.0; }
}  // namespace mvsdet

#include "adapter_sh_table.h"

namespace mvsdet {
namespace {

constexpr int kACam = MVSDET_ADAPTER_CAM;
constexpr int kARot = 24;     // first float of the rotation blocks inside a camera record
constexpr int kAT = 64;       // Gaussians of a block
constexpr int kAThreads = 256;
constexpr int kGeoOut = 19;   // mean 3, covariance 9, scales 3, quaternion 4 (odd: conflict-free rows)
constexpr int kGeoIn = 13;    // g_mean 3, g_covariance 9, one pad

__host__ __device__ constexpr int rot_off(int l) { return l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 10 : l == 3 ? 35 : l == 4 ? 84 : 165; }
int degree_of(int d_sh) { return d_sh == 1 ? 0 : d_sh == 4 ? 1 : d_sh == 9 ? 2 : d_sh == 16 ? 3 : d_sh == 25 ? 4 : -1; }

// ------------------------------------------------------------------------------------------------ cameras
__global__ void adapter_cameras_kernel(const float* __restrict__ ext, int64_t e_view, const float* __restrict__ kin, int64_t k_view,
                                       int64_t k_row, const float* __restrict__ sh_rot, float* __restrict__ cams, int V, int h, int w,
                                       int L) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* E = ext + v * e_view;
    const float* Kp = kin + v * k_view;
    float* c = cams + (int64_t)v * kACam;
    double C[3][3], K[3][3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            C[i][j] = (double)E[i * 4 + j];
            K[i][j] = (double)Kp[i * k_row + j];
            c[i * 3 + j] = E[i * 4 + j];
        }
        c[9 + i] = E[i * 4 + 3];
    }
    // K^-1 by the adjugate
    double Ki[3][3];
    inverse3(K, Ki);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[12 + i * 3 + j] = (float)Ki[i][j];
    // get_scale_multiplier: 0.1 * sum_i (K[:2,:2]^-1 (1/w, 1/h))_i
    const double det2 = K[0][0] * K[1][1] - K[0][1] * K[1][0];
    const double px = 1.0 / (double)w, py = 1.0 / (double)h;
    c[21] = (float)(0.1 * ((K[1][1] * px - K[0][1] * py) / det2 + (K[0][0] * py - K[1][0] * px) / det2));
    c[22] = 0.0f;
    c[23] = 0.0f;
    float* D = c + kARot;
    const int n_rot = rot_off(L + 1);
    for (int i = n_rot; i < kACam - kARot; ++i) D[i] = 0.0f;
    if (sh_rot) {
        for (int i = 0; i < n_rot; ++i) D[i] = sh_rot[(int64_t)v * n_rot + i];
        return;
    }
    D[0] = 1.0f;
    // degree l: D_l^T = B A_l^-1 with B[j][k] = Y_j(C^T d_k)  (sum_j (D c)_j Y_j(C d) = sum_j c_j Y_j(d) at d = C^T d_k)
    for (int l = 1; l <= L; ++l) {
        const int n = 2 * l + 1;
        double B[9][9];
        for (int k = 0; k < n; ++k) {
            const double* d = kShRotDirs + 3 * (kShRotDirOff[l - 1] + k);
            double e[3];
            for (int i = 0; i < 3; ++i) e[i] = C[0][i] * d[0] + C[1][i] * d[1] + C[2][i] * d[2];
            const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            double Y[kShMax];
            sh_basis<double>(e[0] / len, e[1] / len, e[2] / len, (l + 1) * (l + 1), Y);
            for (int j = 0; j < n; ++j) B[j][k] = Y[l * l + j];
        }
        const double* inv = kShRotInv + kShRotInvOff[l - 1];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc += B[j][k] * inv[k * n + i];
                D[rot_off(l) + i * n + j] = (float)acc;
            }
    }
}

// ------------------------------------------------------------------------------------------------ geometry of one Gaussian
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

struct Geo {
    float sig[5];    // sigmoid of the offset (2) and scale (3) features
    float nrm;       // |K^-1 (x, y, 1)|
    float dn[3];     // that direction, normalised (camera space)
    float dw[3];     // C dn
    float base[3];   // s_min + (s_max - s_min) sigmoid
    float sc[3];
    float nq, q[4], qq, two_s;
    float A[9];      // R_q = I + two_s A
    float M[9];      // C R_q
};

// t: the first nine floats of a row; cam: the view's record
__device__ __forceinline__ void geo_forward(const float* t, float depth, const float* __restrict__ cam, int col, int row, int h, int w,
                                            float s_min, float s_max, Geo& g, float* mean, float* cov) {
    for (int i = 0; i < 5; ++i) g.sig[i] = sigmoidf(t[i]);
    const float pw = 1.0f / (float)w, ph = 1.0f / (float)h;
    const float x = ((float)col + 0.5f) / (float)w + (g.sig[0] - 0.5f) * pw;
    const float y = ((float)row + 0.5f) / (float)h + (g.sig[1] - 0.5f) * ph;
    float dir[3];
    for (int i = 0; i < 3; ++i) dir[i] = fmaf(cam[12 + 3 * i + 1], y, cam[12 + 3 * i] * x) + cam[12 + 3 * i + 2];
    g.nrm = sqrtf(fmaf(dir[2], dir[2], fmaf(dir[1], dir[1], dir[0] * dir[0])));
    for (int i = 0; i < 3; ++i) g.dn[i] = dir[i] / g.nrm;
    for (int i = 0; i < 3; ++i) {
        g.dw[i] = fmaf(cam[3 * i + 2], g.dn[2], fmaf(cam[3 * i + 1], g.dn[1], cam[3 * i] * g.dn[0]));
        mean[i] = fmaf(g.dw[i], depth, cam[9 + i]);
    }
    const float dm = depth * cam[21];
    for (int i = 0; i < 3; ++i) {
        g.base[i] = fmaf(s_max - s_min, g.sig[2 + i], s_min);
        g.sc[i] = g.base[i] * dm;
    }
    const float qi = t[5], qj = t[6], qk = t[7], qr = t[8];
    g.nq = sqrtf(fmaf(qr, qr, fmaf(qk, qk, fmaf(qj, qj, qi * qi))));
    const float inv = 1.0f / (g.nq + 1e-8f);
    const float i_ = qi * inv, j_ = qj * inv, k_ = qk * inv, r_ = qr * inv;
    g.q[0] = i_;
    g.q[1] = j_;
    g.q[2] = k_;
    g.q[3] = r_;
    g.qq = fmaf(r_, r_, fmaf(k_, k_, fmaf(j_, j_, i_ * i_))) + 1e-8f;
    g.two_s = 2.0f / g.qq;
    g.A[0] = -(j_ * j_ + k_ * k_);
    g.A[1] = i_ * j_ - k_ * r_;
    g.A[2] = i_ * k_ + j_ * r_;
    g.A[3] = i_ * j_ + k_ * r_;
    g.A[4] = -(i_ * i_ + k_ * k_);
    g.A[5] = j_ * k_ - i_ * r_;
    g.A[6] = i_ * k_ - j_ * r_;
    g.A[7] = j_ * k_ + i_ * r_;
    g.A[8] = -(i_ * i_ + j_ * j_);
    float Rq[9];
    for (int i = 0; i < 9; ++i) Rq[i] = g.two_s * g.A[i];
    Rq[0] += 1.0f;
    Rq[4] += 1.0f;
    Rq[8] += 1.0f;
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 3; ++k)
            g.M[3 * a + k] = fmaf(cam[3 * a + 2], Rq[6 + k], fmaf(cam[3 * a + 1], Rq[3 + k], cam[3 * a] * Rq[k]));
    // covariance = M diag(sc^2) M^T, all nine entries
    const float s2[3] = {g.sc[0] * g.sc[0], g.sc[1] * g.sc[1], g.sc[2] * g.sc[2]};
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            const float val = fmaf(g.M[3 * a + 2] * g.M[3 * b + 2], s2[2],
                                   fmaf(g.M[3 * a + 1] * g.M[3 * b + 1], s2[1], g.M[3 * a] * g.M[3 * b] * s2[0]));
            cov[3 * a + b] = val;
            cov[3 * b + a] = val;
        }
}

// chain rule of geo_forward: gm (3), gc (3x3, any) -> gt (9), the gradient of the row's first nine floats; returns d / d depth
__device__ __forceinline__ float geo_backward(const Geo& g, float depth, const float* __restrict__ cam, int h, int w, float s_min,
                                              float s_max, const float* gm, const float* gc, float* gt) {
    float gd = 0.0f;
    // covariance = M S2 M^T
    float Gs[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Gs[3 * a + b] = gc[3 * a + b] + gc[3 * b + a];
    const float s2[3] = {g.sc[0] * g.sc[0], g.sc[1] * g.sc[1], g.sc[2] * g.sc[2]};
    float gM[9], gsc[3];
    for (int k = 0; k < 3; ++k) {
        float acc = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float u = fmaf(Gs[3 * a + 2], g.M[6 + k], fmaf(Gs[3 * a + 1], g.M[3 + k], Gs[3 * a] * g.M[k]));   // (Gs M)[a][k]
            gM[3 * a + k] = u * s2[k];
            acc = fmaf(u, g.M[3 * a + k], acc);
        }
        gsc[k] = acc * g.sc[k];      // sum_ab G_ab M_ak M_bk = (M^T Gs M)_kk / 2, times 2 sc
    }
    // M = C R_q
    float gR[9];
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 3; ++k) gR[3 * a + k] = fmaf(cam[6 + a], gM[6 + k], fmaf(cam[3 + a], gM[3 + k], cam[a] * gM[k]));
    // R_q = I + two_s A(q)
    float g_two_s = 0.0f, gA[9];
    for (int i = 0; i < 9; ++i) {
        g_two_s = fmaf(gR[i], g.A[i], g_two_s);
        gA[i] = g.two_s * gR[i];
    }
    const float i_ = g.q[0], j_ = g.q[1], k_ = g.q[2], r_ = g.q[3];
    float gq[4];
    gq[0] = (gA[1] + gA[3]) * j_ + (gA[2] + gA[6]) * k_ + (gA[7] - gA[5]) * r_ - 2.0f * i_ * (gA[4] + gA[8]);
    gq[1] = (gA[1] + gA[3]) * i_ + (gA[5] + gA[7]) * k_ + (gA[2] - gA[6]) * r_ - 2.0f * j_ * (gA[0] + gA[8]);
    gq[2] = (gA[2] + gA[6]) * i_ + (gA[5] + gA[7]) * j_ + (gA[3] - gA[1]) * r_ - 2.0f * k_ * (gA[0] + gA[4]);
    gq[3] = (gA[3] - gA[1]) * k_ + (gA[2] - gA[6]) * j_ + (gA[7] - gA[5]) * i_;
    const float g_qq = -(g.two_s / g.qq) * g_two_s;
    for (int i = 0; i < 4; ++i) gq[i] = fmaf(2.0f * g.q[i], g_qq, gq[i]);
    // q = q_raw / (|q_raw| + eps)
    const float inv = 1.0f / (g.nq + 1e-8f);
    const float dot = (gq[0] * g.q[0] + gq[1] * g.q[1] + gq[2] * g.q[2] + gq[3] * g.q[3]);   // gq . q_raw * inv
    // d q_a / d raw_b = inv delta_ab - raw_a raw_b inv^2 / nq = inv (delta_ab - q_a raw_b inv / nq) ; raw_b inv = q_b
    // nq == 0 (a zero quaternion, or squares that underflowed): the projection term vanishes against inv gq there and must not divide
    // by nq; what is left is torch's subgradient of the norm at 0.  + 0.0f: a zero quaternion's gradient is +0 in every component
    for (int i = 0; i < 4; ++i) {
        const float full = inv * (gq[i] - dot * g.q[i] * ((g.nq + 1e-8f) / g.nq));
        gt[5 + i] = g.nq > 0.0f ? full : inv * gq[i] + 0.0f;
    }
    // scales
    const float dm = depth * cam[21];
    for (int k = 0; k < 3; ++k) {
        gt[2 + k] = gsc[k] * dm * (s_max - s_min) * g.sig[2 + k] * (1.0f - g.sig[2 + k]);
        gd = fmaf(gsc[k], g.base[k] * cam[21], gd);
    }
    // mean = origin + (C dn) depth
    float gdn[3];
    for (int i = 0; i < 3; ++i) gd = fmaf(gm[i], g.dw[i], gd);
    for (int i = 0; i < 3; ++i) gdn[i] = (cam[6 + i] * gm[2] + cam[3 + i] * gm[1] + cam[i] * gm[0]) * depth;
    const float along = gdn[0] * g.dn[0] + gdn[1] * g.dn[1] + gdn[2] * g.dn[2];
    float gdir[3];
    for (int i = 0; i < 3; ++i) gdir[i] = (gdn[i] - g.dn[i] * along) / g.nrm;
    const float gx = cam[12] * gdir[0] + cam[15] * gdir[1] + cam[18] * gdir[2];
    const float gy = cam[13] * gdir[0] + cam[16] * gdir[1] + cam[19] * gdir[2];
    gt[0] = gx * (1.0f / (float)w) * g.sig[0] * (1.0f - g.sig[0]);
    gt[1] = gy * (1.0f / (float)h) * g.sig[1] * (1.0f - g.sig[1]);
    return gd;
}

// sh_mask of the adapter: 1 at degree 0, 0.1 * 0.25^l on degree l
__device__ __forceinline__ constexpr float sh_mask(int l) {
    return l == 0 ? 1.0f : l == 1 ? 0.025f : l == 2 ? 0.00625f : l == 3 ? 0.0015625f : 0.000390625f;
}

// out = blockdiag(D_l) (mask * c), or with TRANSPOSE: out = mask * blockdiag(D_l)^T c.  D: the view's blocks (uniform address)
template <int L, bool TRANSPOSE>
__device__ __forceinline__ void rotate_harmonics(const float* __restrict__ D, const float* c, float* out) {
#pragma unroll
    for (int l = 0; l <= L; ++l) {
        const int n = 2 * l + 1, first = l * l, off = rot_off(l);
        const float m = sh_mask(l);
#pragma unroll
        for (int i = 0; i < n; ++i) {
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const float d = TRANSPOSE ? D[off + j * n + i] : D[off + i * n + j];
                acc = fmaf(d, TRANSPOSE ? c[first + j] : m * c[first + j], acc);
            }
            out[first + i] = TRANSPOSE ? m * acc : acc;
        }
    }
}

template <int L>
__global__ __launch_bounds__(kAThreads) void adapter_forward_kernel(const float* __restrict__ raw, int64_t r_view, int64_t r_row,
                                                                    const float* __restrict__ depth, const float* __restrict__ cams,
                                                                    float* __restrict__ means, float* __restrict__ covs,
                                                                    float* __restrict__ harm, float* __restrict__ scales,
                                                                    float* __restrict__ rots, int N, int h, int w, int S, float s_min,
                                                                    float s_max) {
    constexpr int DSH = (L + 1) * (L + 1), ROW = 9 + 3 * DSH, LROW = ROW | 1;
    __shared__ float tile[kAT * LROW];
    __shared__ float geo[kAT * kGeoOut];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int g0 = blockIdx.x * kAT;
    const int cnt = min(kAT, N - g0);
    const float* cam = cams + (int64_t)v * kACam;
    const float* src = raw + (int64_t)v * r_view + (int64_t)g0 * r_row;
    for (int idx = tid; idx < cnt * ROW; idx += kAThreads) {
        const int row = idx / ROW, k = idx - row * ROW;
        tile[row * LROW + k] = src[(int64_t)row * r_row + k];
    }
    __syncthreads();
    const int part = tid >> 6, gl = tid & (kAT - 1);
    if (gl < cnt) {
        if (part < 3) {
            float* p = tile + gl * LROW + 9 + part * DSH;
            float c[DSH], out[DSH];
#pragma unroll
            for (int j = 0; j < DSH; ++j) c[j] = p[j];
            rotate_harmonics<L, false>(cam + kARot, c, out);
#pragma unroll
            for (int j = 0; j < DSH; ++j) p[j] = out[j];
        } else {
            const int r = (g0 + gl) / S;
            Geo g;
            float* o = geo + gl * kGeoOut;
            geo_forward(tile + gl * LROW, depth[(int64_t)v * (N / S) + r], cam, r % w, r / w, h, w, s_min, s_max, g, o, o + 3);
            for (int i = 0; i < 3; ++i) o[12 + i] = g.sc[i];
            for (int i = 0; i < 4; ++i) o[15 + i] = g.q[i];
        }
    }
    __syncthreads();
    const int64_t gbase = (int64_t)v * N + g0;
    for (int idx = tid; idx < cnt * 3 * DSH; idx += kAThreads) {
        const int row = idx / (3 * DSH), k = idx - row * (3 * DSH);
        harm[gbase * (3 * DSH) + idx] = tile[row * LROW + 9 + k];
    }
    for (int idx = tid; idx < cnt * 9; idx += kAThreads) {
        const int row = idx / 9, k = idx - row * 9;
        covs[gbase * 9 + idx] = geo[row * kGeoOut + 3 + k];
    }
    for (int idx = tid; idx < cnt * 3; idx += kAThreads) {
        const int row = idx / 3, k = idx - row * 3;
        means[gbase * 3 + idx] = geo[row * kGeoOut + k];
        if (scales) scales[gbase * 3 + idx] = geo[row * kGeoOut + 12 + k];
    }
    if (rots)
        for (int idx = tid; idx < cnt * 4; idx += kAThreads) rots[gbase * 4 + idx] = geo[(idx >> 2) * kGeoOut + 15 + (idx & 3)];
}

template <int L>
__global__ __launch_bounds__(kAThreads) void adapter_backward_kernel(const float* __restrict__ raw, int64_t r_view, int64_t r_row,
                                                                     const float* __restrict__ depth, const float* __restrict__ cams,
                                                                     const float* __restrict__ g_means, const float* __restrict__ g_covs,
                                                                     const float* __restrict__ g_harm, float* __restrict__ g_raw,
                                                                     int64_t g_view, int64_t g_row, float* __restrict__ g_depth, int N,
                                                                     int h, int w, int S, float s_min, float s_max) {
    constexpr int DSH = (L + 1) * (L + 1), ROW = 9 + 3 * DSH, LROW = ROW | 1;
    __shared__ float tile[kAT * LROW];     // g_harmonics in, the whole row of g_raw out
    __shared__ float head[kAT * 9];        // the first nine floats of the rows of raw
    __shared__ float gin[kAT * kGeoIn];
    const int v = blockIdx.y, tid = threadIdx.x;
    const int g0 = blockIdx.x * kAT;
    const int cnt = min(kAT, N - g0);
    const float* cam = cams + (int64_t)v * kACam;
    const float* src = raw + (int64_t)v * r_view + (int64_t)g0 * r_row;
    const int64_t gbase = (int64_t)v * N + g0;
    for (int idx = tid; idx < cnt * 3 * DSH; idx += kAThreads) {
        const int row = idx / (3 * DSH), k = idx - row * (3 * DSH);
        tile[row * LROW + 9 + k] = g_harm ? g_harm[gbase * (3 * DSH) + idx] : 0.0f;
    }
    for (int idx = tid; idx < cnt * 9; idx += kAThreads) {
        const int row = idx / 9, k = idx - row * 9;
        head[idx] = src[(int64_t)row * r_row + k];
        gin[row * kGeoIn + 3 + k] = g_covs ? g_covs[gbase * 9 + idx] : 0.0f;
    }
    for (int idx = tid; idx < cnt * 3; idx += kAThreads) {
        const int row = idx / 3, k = idx - row * 3;
        gin[row * kGeoIn + k] = g_means ? g_means[gbase * 3 + idx] : 0.0f;
    }
    __syncthreads();
    const int part = tid >> 6, gl = tid & (kAT - 1);
    if (gl < cnt) {
        if (part < 3) {
            float* p = tile + gl * LROW + 9 + part * DSH;
            float c[DSH], out[DSH];
#pragma unroll
            for (int j = 0; j < DSH; ++j) c[j] = p[j];
            rotate_harmonics<L, true>(cam + kARot, c, out);
#pragma unroll
            for (int j = 0; j < DSH; ++j) p[j] = out[j];
        } else {
            const int r = (g0 + gl) / S;
            const float d = depth[(int64_t)v * (N / S) + r];
            Geo g;
            float mean[3], cov[9];
            geo_forward(head + gl * 9, d, cam, r % w, r / w, h, w, s_min, s_max, g, mean, cov);
            g_depth[gbase + gl] = geo_backward(g, d, cam, h, w, s_min, s_max, gin + gl * kGeoIn, gin + gl * kGeoIn + 3, tile + gl * LROW);
        }
    }
    __syncthreads();
    float* dst = g_raw + (int64_t)v * g_view + (int64_t)g0 * g_row;
    for (int idx = tid; idx < cnt * ROW; idx += kAThreads) {
        const int row = idx / ROW, k = idx - row * ROW;
        dst[(int64_t)row * g_row + k] = tile[row * LROW + k];
    }
}

int check_sizes(const char* name, int V, int h, int w, int S, int d_sh) {
    MVS_REQUIRE(degree_of(d_sh) >= 0, "%s: d_sh = %d must be 1, 4, 9, 16 or 25", name, d_sh);
    MVS_REQUIRE(V > 0 && V <= 65535 && h > 0 && w > 0 && S > 0, "%s: bad sizes V=%d (at most 65535) h=%d w=%d S=%d", name, V, h, w, S);
    const long long N = (long long)h * w * S;
    MVS_REQUIRE(N * (10 + 3 * d_sh) < (1ll << 31) && (long long)V * N * 3 * d_sh < (1ll << 31),
                "%s: V=%d h=%d w=%d S=%d d_sh=%d exceeds the limits (h w S (10 + 3 d_sh) and V h w S 3 d_sh below 2^31)", name, V, h, w, S, d_sh);
    return MVSDET_OK;
}

}  // namespace
}  // namespace mvsdet

using namespace mvsdet;

extern "C" int mvsdet_adapter_cameras_f32(const float* extrinsics, int64_t ext_view_stride, const float* intrinsics, int64_t k_view_stride,
                                          int64_t k_row_stride, const float* sh_rot, float* cams, int V, int h, int w, int d_sh,
                                          mvsdet_stream_t stream) {
    MVS_REQUIRE(extrinsics && intrinsics && cams, "adapter_cameras: NULL pointer");
    MVS_REQUIRE(degree_of(d_sh) >= 0, "adapter_cameras: d_sh = %d must be 1, 4, 9, 16 or 25", d_sh);
    MVS_REQUIRE(V > 0 && h > 0 && w > 0 && k_row_stride >= 3, "adapter_cameras: bad sizes V=%d h=%d w=%d, intrinsics rows of %lld elements", V,
                h, w, (long long)k_row_stride);
    hipLaunchKernelGGL(adapter_cameras_kernel, dim3((V + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, extrinsics, ext_view_stride,
                       intrinsics, k_view_stride, k_row_stride, sh_rot, cams, V, h, w, degree_of(d_sh));
    MVS_LAUNCH_CHECK("adapter_cameras");
    return MVSDET_OK;
}

extern "C" int mvsdet_adapter_forward_f32(const float* raw, int64_t raw_view_stride, int64_t raw_row_stride, const float* depth,
                                          const float* cams, float* means, float* covariances, float* harmonics, float* scales,
                                          float* rotations, int V, int h, int w, int S, int d_sh, float scale_min, float scale_max,
                                          mvsdet_stream_t stream) {
    MVS_REQUIRE(raw && depth && cams && means && covariances && harmonics, "adapter_forward: NULL pointer");
    MVS_REQUIRE((scales == nullptr) == (rotations == nullptr), "adapter_forward: scales and rotations come together or not at all");
    if (int rc = check_sizes("adapter_forward", V, h, w, S, d_sh)) return rc;
    MVS_REQUIRE(raw_row_stride >= 9 + 3 * d_sh, "adapter_forward: rows of %d floats %lld apart", 9 + 3 * d_sh, (long long)raw_row_stride);
    const int N = h * w * S;
    const dim3 grid((N + kAT - 1) / kAT, V), block(kAThreads);
#define ADAPTER_FWD(L)                                                                                                               \
    hipLaunchKernelGGL(adapter_forward_kernel<L>, grid, block, 0, (hipStream_t)stream, raw, raw_view_stride, raw_row_stride, depth, \
                       cams, means, covariances, harmonics, scales, rotations, N, h, w, S, scale_min, scale_max)
    switch (degree_of(d_sh)) {
        case 0: ADAPTER_FWD(0); break;
        case 1: ADAPTER_FWD(1); break;
        case 2: ADAPTER_FWD(2); break;
        case 3: ADAPTER_FWD(3); break;
        default: ADAPTER_FWD(4); break;
    }
#undef ADAPTER_FWD
    MVS_LAUNCH_CHECK("adapter_forward");
    return MVSDET_OK;
}

extern "C" int mvsdet_adapter_backward_f32(const float* raw, int64_t raw_view_stride, int64_t raw_row_stride, const float* depth,
                                           const float* cams, const float* g_means, const float* g_covariances, const float* g_harmonics,
                                           float* g_raw, int64_t g_raw_view_stride, int64_t g_raw_row_stride, float* g_depth, int V, int h,
                                           int w, int S, int d_sh, float scale_min, float scale_max, mvsdet_stream_t stream) {
    MVS_REQUIRE(raw && depth && cams && g_raw && g_depth, "adapter_backward: NULL pointer");
    if (int rc = check_sizes("adapter_backward", V, h, w, S, d_sh)) return rc;
    MVS_REQUIRE(raw_row_stride >= 9 + 3 * d_sh && g_raw_row_stride >= 9 + 3 * d_sh, "adapter_backward: rows of %d floats %lld and %lld apart",
                9 + 3 * d_sh, (long long)raw_row_stride, (long long)g_raw_row_stride);
    const int N = h * w * S;
    const dim3 grid((N + kAT - 1) / kAT, V), block(kAThreads);
#define ADAPTER_BWD(L)                                                                                                                \
    hipLaunchKernelGGL(adapter_backward_kernel<L>, grid, block, 0, (hipStream_t)stream, raw, raw_view_stride, raw_row_stride, depth, \
                       cams, g_means, g_covariances, g_harmonics, g_raw, g_raw_view_stride, g_raw_row_stride, g_depth, N, h, w, S,    \
                       scale_min, scale_max)
    switch (degree_of(d_sh)) {
        case 0: ADAPTER_BWD(0); break;
        case 1: ADAPTER_BWD(1); break;
        case 2: ADAPTER_BWD(2); break;
        case 3: ADAPTER_BWD(3); break;
        default: ADAPTER_BWD(4); break;
    }
#undef ADAPTER_BWD
    MVS_LAUNCH_CHECK("adapter_backward");
    return MVSDET_OK;
}
