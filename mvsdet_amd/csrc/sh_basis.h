// Real spherical harmonics of degree 0..4 along a unit direction, as the Gaussian rasteriser evaluates them (csrc/splat.hip).
// Degrees 0..3: the constants and signs published with Kerbl et al. 2023.  Degree 4: the nine real l = 4 harmonics in the same sign
// convention (odd |m| negative).  ONE copy of the polynomials: the forward evaluates them on float, the backward on Dual3, which
// carries the three partial derivatives along, so the derivative cannot drift from the value.
#pragma once
#include <hip/hip_runtime.h>

namespace mvsdet {

constexpr int kShMax = 25;   // coefficients of degree 4

struct Dual3 {
    float v, dx, dy, dz;
};
__host__ __device__ __forceinline__ Dual3 operator+(Dual3 a, Dual3 b) { return {a.v + b.v, a.dx + b.dx, a.dy + b.dy, a.dz + b.dz}; }
__host__ __device__ __forceinline__ Dual3 operator-(Dual3 a, Dual3 b) { return {a.v - b.v, a.dx - b.dx, a.dy - b.dy, a.dz - b.dz}; }
__host__ __device__ __forceinline__ Dual3 operator*(Dual3 a, Dual3 b) {
    return {a.v * b.v, a.dx * b.v + a.v * b.dx, a.dy * b.v + a.v * b.dy, a.dz * b.v + a.v * b.dz};
}
__host__ __device__ __forceinline__ Dual3 operator*(float s, Dual3 a) { return {s * a.v, s * a.dx, s * a.dy, s * a.dz}; }
__host__ __device__ __forceinline__ Dual3 operator-(Dual3 a, float s) { return {a.v - s, a.dx, a.dy, a.dz}; }

template <class T>
__host__ __device__ __forceinline__ T sh_one(T like);
template <>
__host__ __device__ __forceinline__ float sh_one<float>(float) { return 1.0f; }
template <>
__host__ __device__ __forceinline__ Dual3 sh_one<Dual3>(Dual3) { return {1.0f, 0.0f, 0.0f, 0.0f}; }

// out[0 .. n) for n in {1, 4, 9, 16, 25}
template <class T>
__host__ __device__ __forceinline__ void sh_basis(T x, T y, T z, int n, T* out) {
    out[0] = 0.28209479177387814f * sh_one(x);
    if (n < 4) return;
    out[1] = -0.4886025119029199f * y;
    out[2] = 0.4886025119029199f * z;
    out[3] = -0.4886025119029199f * x;
    if (n < 9) return;
    const T xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    out[4] = 1.0925484305920792f * xy;
    out[5] = -1.0925484305920792f * yz;
    out[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
    out[7] = -1.0925484305920792f * xz;
    out[8] = 0.5462742152960396f * (xx - yy);
    if (n < 16) return;
    out[9] = -0.5900435899266435f * (y * (3.0f * xx - yy));
    out[10] = 2.890611442640554f * (xy * z);
    out[11] = -0.4570457994644658f * (y * (4.0f * zz - xx - yy));
    out[12] = 0.3731763325901154f * (z * (2.0f * zz - 3.0f * xx - 3.0f * yy));
    out[13] = -0.4570457994644658f * (x * (4.0f * zz - xx - yy));
    out[14] = 1.445305721320277f * (z * (xx - yy));
    out[15] = -0.5900435899266435f * (x * (xx - 3.0f * yy));
    if (n < 25) return;
    out[16] = 2.5033429417967046f * (xy * (xx - yy));
    out[17] = -1.7701307697799304f * (yz * (3.0f * xx - yy));
    out[18] = 0.9461746957575601f * (xy * (7.0f * zz - 1.0f));
    out[19] = -0.6690465435572892f * (yz * (7.0f * zz - 3.0f));
    out[20] = 0.10578554691520431f * (zz * (35.0f * zz - 30.0f) - (-3.0f));
    out[21] = -0.6690465435572892f * (xz * (7.0f * zz - 3.0f));
    out[22] = 0.47308734787878004f * ((xx - yy) * (7.0f * zz - 1.0f));
    out[23] = -1.7701307697799304f * (xz * (xx - 3.0f * yy));
    out[24] = 0.6258357354491761f * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
}

}  // namespace mvsdet
