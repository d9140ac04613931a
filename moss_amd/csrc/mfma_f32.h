// mfma_f32.h -- the f32 matrix-core tile (v_mfma_f32_32x32x2_f32: a 32 x 32 block of C/D in 16 registers per lane) as the fused-op
// GEMMs use it (lbs_weight_net.hip, lpips.hip).  Lane l holds column l & 31; `half` = l >> 5 selects the k of A/B and the rows of C/D.
#pragma once
#include <hip/hip_runtime.h>

namespace moss {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }   // C/D: col = lane & 31

__device__ __forceinline__ f32x16 splat(float v)
{
    f32x16 r;
#pragma unroll
    for (int i = 0; i < 16; i++) r[i] = v;
    return r;
}

// acc += A B over this lane's four consecutive k (eight per wave: 4 * half + 0..3).  av: float4 or a 4-vector; bv: a 4-vector or float[4]
template <typename A, typename B>
__device__ __forceinline__ void mfma4(f32x16& acc, const A& av, const B& bv)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[3], acc, 0, 0, 0);
}

}  // namespace moss
