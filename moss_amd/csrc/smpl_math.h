// smpl_math.h -- device helpers shared by the per-frame SMPL kernels (smpl_frame.hip, frame_bounds.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace moss {

// the reference's Rodrigues (gaussian_model.py:945-963): angle = |r + 1e-8|, n = r / angle, R = I + sin K + (1 - cos) K K
__device__ __forceinline__ void sf_rodrigues(const float* r, float* R)
{
    const float x = r[0], y = r[1], z = r[2];
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float nx = x / angle, ny = y / angle, nz = z / angle;
    const float s = sinf(angle), c = 1.0f - cosf(angle);
    R[0] = 1.0f - c * (ny * ny + nz * nz); R[1] = c * (nx * ny) - s * nz;          R[2] = c * (nx * nz) + s * ny;
    R[3] = c * (nx * ny) + s * nz;          R[4] = 1.0f - c * (nx * nx + nz * nz); R[5] = c * (ny * nz) - s * nx;
    R[6] = c * (nx * nz) - s * ny;          R[7] = c * (ny * nz) + s * nx;          R[8] = 1.0f - c * (nx * nx + ny * ny);
}

}  // namespace moss
