// kl_math.h -- build_rotation (utils/general_utils.py:79-100) as a device function, shared by neighbour_kl_kernel (densify.hip) and the row
// kernel of the densify decision (densify_decision.hip).  The KL itself has ONE body, neighbour_kl_kernel: the decision's selection
// launches that kernel (launch_neighbour_kl, common.h) instead of restating its arithmetic, because the same statements compiled in
// another kernel are packed and contracted in another order and differ in the last bits.
#pragma once
#include <hip/hip_runtime.h>

namespace moss {

__device__ __forceinline__ void rotation_of(const float* __restrict__ q4, float R[3][3])     // utils/general_utils.py:79-100
{
    const float a = q4[0], b = q4[1], c = q4[2], d = q4[3];
    const float inv = 1.0f / sqrtf(a * a + b * b + c * c + d * d);
    const float r = a * inv, x = b * inv, y = c * inv, z = d * inv;
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z);       R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z);       R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y);       R[2][1] = 2.f * (y * z + r * x);       R[2][2] = 1.f - 2.f * (x * x + y * y);
}

}  // namespace moss
