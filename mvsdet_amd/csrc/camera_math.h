// The float64 inverse of a 3x3 matrix that the one-thread-per-view camera kernels share (splat_cameras_kernel, adapter_cameras_kernel,
// photo_geometry_kernel): adjugate over determinant, the determinant expanded along the first row.  ONE copy of the twelve
// expressions, in one order: the library is built with -ffp-contract=off, so every caller gets the same bits.  A singular matrix
// gives inf / NaN, as the division says; nothing is tested.
#pragma once
#include <hip/hip_runtime.h>

namespace mvsdet {

__host__ __device__ inline void inverse3(const double (*M)[3], double (*inv)[3]) {
    const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2];
    const double c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
    inv[0][0] = c00 / det;
    inv[1][0] = c01 / det;
    inv[2][0] = c02 / det;
    inv[0][1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) / det;
    inv[1][1] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) / det;
    inv[2][1] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) / det;
    inv[0][2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) / det;
    inv[1][2] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) / det;
    inv[2][2] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) / det;
}

}  // namespace mvsdet
