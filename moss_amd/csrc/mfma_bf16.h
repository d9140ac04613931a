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

// a float32 as two bf16: hi = rne(a), lo = rne(a - hi).  The subtraction is exact in float32 (hi is a's leading 8 bits), so hi + lo
// carries about 16 bits of a: |lo| <= 2^-8 |a| and |a - hi - lo| <= 2^-17 |a|.  (A lo below bf16's normal range may be flushed by the
// matrix core.)
__device__ __forceinline__ void split_bf16(float a, __bf16& hi, __bf16& lo)
{
    hi = (__bf16)a;
    lo = (__bf16)(a - (float)hi);
}

template <typename V>
__device__ __forceinline__ void split_bf16x4(const V& v, bf16x4& hi, bf16x4& lo)
{
    hi = to_bf16x4(v);
    lo = bf16x4{(__bf16)(v.x - (float)hi.x), (__bf16)(v.y - (float)hi.y), (__bf16)(v.z - (float)hi.z), (__bf16)(v.w - (float)hi.w)};
}

// a lane's eight k of one operand, split
__device__ __forceinline__ void split_bf16x8(const float (&v)[8], bf16x8& hi, bf16x8& lo)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        hi[i] = (__bf16)v[i];
        lo[i] = (__bf16)(v[i] - (float)hi[i]);
    }
}

// acc += A B over the wave's sixteen k of this step
__device__ __forceinline__ void mfma16(f32x16& acc, const bf16x8& av, const bf16x8& bv)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
}

// acc += lo(A) hi(B) + hi(A) lo(B) + hi(A) hi(B): the three-product form of a float32 product (lo lo is dropped), small terms first
__device__ __forceinline__ void mfma16x3(f32x16& acc, const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl)
{
    mfma16(acc, al, bh);
    mfma16(acc, ah, bl);
    mfma16(acc, ah, bh);
}

}  // namespace moss
