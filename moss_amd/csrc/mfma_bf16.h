// mfma_bf16.h -- the bf16-operand matrix-core tile (v_mfma_f32_32x32x16_bf16) beside mfma_f32.h's: the same 32 x 32 block of C/D in 16
// float32 registers per lane (acc_row, splat carry over), fed 16 k per instruction.  Lane l supplies row (A) / column (B) l & 31 and
// the eight consecutive k values 8 * (l >> 5) .. + 7: with k contiguous in memory that is one 16-byte read.  The products are exact
// (bf16 x bf16 fits float32), the accumulation is float32.
#pragma once
#include "mfma_f32.h"

namespace moss {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// four floats rounded to nearest even (v_cvt_pk_bf16_f32), 8 bytes
template <typename V>
__device__ __forceinline__ bf16x4 to_bf16x4(const V& v)
{
    return bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

// acc += A B over the wave's sixteen k of this step
__device__ __forceinline__ void mfma16(f32x16& acc, const bf16x8& av, const bf16x8& bv)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
}

}  // namespace moss
