// wave.h -- reductions and a scan over the 64 lanes of a wave, and the ordered-integer keys of floats that go with the min / max,
// shared by the fused-op kernels.  The reductions are xor butterflies: every lane ends with the same bits.  (blend.hip,
// preprocess.hip, binning.hip and optim.hip keep their own shuffles: those are tuned in place.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace moss {

template <typename T>                  // (float, double or int)
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// inclusive prefix sum over the wave's lanes (lane l: the sum of lanes 0 .. l)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d); if ((int)(threadIdx.x & 63) >= d) v += t; }
    return v;
}

// float <-> unsigned key with the same order (for atomicMin / atomicMax on floats of either sign)
__device__ __forceinline__ uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

}  // namespace moss
