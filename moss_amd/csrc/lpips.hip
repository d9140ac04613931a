// lpips.hip -- MOSS's LPIPS term, LPIPS.forward with net_type='vgg' (lpipsPyTorch/modules/lpips.py:31-37, networks.py:49-62,87-95,
// utils.py:5-7), and its gradient w.r.t. the first image (include/moss_raster.h moss_lpips_vgg_forward / _backward).
//
//     z = (img - shift) / scale;  VGG16 features[0:30]: 13 x (conv 3x3 pad 1 + bias + ReLU), a 2x2 max-pool after conv 1_2, 2_2, 3_3, 4_3
//     tap l (after ReLU 1_2, 2_2, 3_3, 4_3, 5_3):  n = f / (sqrt(sum_c f^2) + 1e-10),  term_l = mean_p sum_c lin_l[c] (nx - ny)^2
//     out = sum_l term_l
// The weights are frozen and the second image is the ground truth, so the only gradient is d out / d x, and it needs no layer input:
// a ReLU passes its gradient where its output was positive (one BIT per activation), a pool where its winner sat (two bits per
// pooled activation), and the five tap terms enter through d term_l / d fx, which the forward's tap kernel writes itself while it
// has fx and fy in registers (one tensor per tap, of x's size: the feature maps of y are never kept).
//
// Activations are channels-last, both images one batch of two: row m = img * H W + y W + x, C floats per row.
//   conv3x3_mfma_kernel -- THE convolution, an implicit GEMM (M = rows, N = Cout, K = 9 Cin ordered tap-major) on the f32-input matrix
//     cores (v_mfma_f32_32x32x2_f32: exact float32, an ordered fmaf chain).  It runs the twelve wide layers forward (epilogue: bias,
//     ReLU, the sign bits by one ballot per accumulator register) and, on weights flipped and transposed once at construction, their
//     data gradients (epilogue: the ReLU bits of the layer below, or nothing where a pool follows below).  A workgroup of four waves
//     stages a 64-deep slice of K -- one tap, 64 consecutive channels: 256 contiguous bytes per row -- of both operands in LDS (row
//     stride 68 floats = 4 mod 64: the float4 reads of 32 lanes hit 32 different bank groups) while the NEXT slice is already on its
//     way from L2 into registers; a wave owns a 32 x 64 block (two accumulators share every A read).  Two shapes: 128 rows x 64
//     channels per workgroup (a wave per 32 rows), and, for the deep layers whose few rows would leave most CUs idle, 32 rows x 64
//     channels with the four waves splitting every K slice, their partial blocks summed in wave order through LDS.
//   conv3x3_bf16_kernel -- the same convolution with both operands rounded to bf16 and float32 sums (v_mfma_f32_32x32x16_bf16), behind
//     moss_lpips_vgg_forward_bf16 / _backward_bf16: an opt-in form of the TRAINING term.  Same shapes, modes and epilogue; see there.
//   conv3x3_bf16x3_kernel -- the same convolution with each operand split into two bf16 and three products per product (about 16 bits
//     of every operand), behind moss_lpips_vgg_forward_bf16x3 / _backward_bf16x3: between the two in cost and in accuracy; see there.
//   conv_first_kernel / conv_first_backward_kernel -- conv 1_1 (Cin = 3, K = 27) and its adjoint on the VALU, with the z-score, the
//     crop offset read from the device and the planar (3,H,W) layout of the public tensors.
//   pool_kernel, tap_kernel, unpool_tap_kernel, reduce_kernel -- see each.
//   conv_first_one_kernel, tap_ref_kernel -- the one-image forms behind moss_lpips_vgg_reference (the ground truth's tapped activations,
//     once, into a caller's block) and moss_lpips_vgg_forward_ref (the forward on x alone, y's activations read from that block): the
//     wide convolutions, the pool and the reduction are the kernels above at nimg = 1, the backward is untouched (forward_launches).
// Every sum has a fixed order and there is no atomic: results are bitwise reproducible.  Every element of dL_dx is written.
//
// With a CAPACITY (moss_lpips_vgg_args.cap_H, cap_W) the crop's size is not a launch argument: every kernel reads {w, h} from the
// device rectangle itself (struct Dyn, actual_size) and derives its level's H_l = h >> l, W_l = w >> l, M and HW from them.  The host
// sizes the grids and the regions of `saved` and `workspace` for the capacity; inside a region the rows are compact at the ACTUAL
// size (img * H_l * W_l + y * W_l + x), exactly the layout of the static call at h x w, and a workgroup whose rows all lie beyond
// the actual M returns before its first barrier.  The arithmetic is the static call's; launch_conv picks the kernel shape from the
// capacity's M, so the result equals the static call's bit for bit when every layer gets the same shape in both, and to float32
// summation order otherwise (include/moss_raster.h).
#include "common.h"
#include "mfma_bf16.h"
#include "mfma_f32.h"
#include "wave.h"

namespace moss {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NCONV = MOSS_LPIPS_VGG_CONVS, NTAP = MOSS_LPIPS_VGG_TAPS;
constexpr int CONV_COUT[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int CONV_LEVEL[NCONV] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int TAP_CONV[NTAP] = {1, 3, 6, 9, 12};
constexpr int TAP_C[NTAP] = {64, 128, 256, 512, 512};
constexpr int WG = 256;
constexpr int KC = 64, LD = KC + 4, BN = 64;             // K slice, LDS row stride (floats), output channels per workgroup
constexpr float NORM_EPS = 1e-10f;
enum { MODE_FWD, MODE_BWD_MASK, MODE_BWD_PLAIN };

// The crop's size on the device.  cap_H == 0: the static call, the sizes are the launch's.  Otherwise rect[2], rect[3] = {w, h}, clamped
// into [16, capacity] -- for memory safety only, the host validates what it can see -- and halved `level` times.
struct Dyn {
    const int* rect;
    int cap_H, cap_W, level;
};

__device__ __forceinline__ void actual_size(const Dyn& d, int& H, int& W)
{
    if (d.cap_H > 0) {
        H = min(max(d.rect[3], 16), d.cap_H) >> d.level;
        W = min(max(d.rect[2], 16), d.cap_W) >> d.level;
    }
}

// where the crop starts in the frame: the rectangle's corner, moved so that the crop fits
__device__ __forceinline__ int2 crop_origin(const int* __restrict__ rect, int H, int W, int FH, int FW)
{
    int2 o = make_int2(0, 0);
    if (rect) {
        o.x = min(max(rect[0], 0), FW - W);
        o.y = min(max(rect[1], 0), FH - H);
    }
    return o;
}

// ---- the weights, once ---------------------------------------------------------------------------------------------------------------
// w (Cout,Cin,3,3) -> fwd [Cout][tap][Cin] and bwd [Cin][flipped tap][Cout]: d in[q][ci] = sum d out[q + (ky' - 1, kx' - 1)][co] bwd[ci][ky' kx'][co]
// T float, or __bf16: rounded to nearest even, once
template <typename T>
__global__ void __launch_bounds__(WG)
pack_weights_kernel(int cin, int cout, const float* __restrict__ w, T* __restrict__ fwd, T* __restrict__ bwd)
{
    const int idx = blockIdx.x * WG + threadIdx.x;
    if (idx >= cout * cin * 9) return;
    const int tap = idx % 9, i = (idx / 9) % cin, o = idx / (9 * cin);
    const T v = (T)w[idx];
    fwd[((size_t)o * 9 + tap) * cin + i] = v;
    bwd[((size_t)i * 9 + (8 - tap)) * cout + o] = v;
}

// the split packing: each array two planes of n = cout cin 9 values in the layouts above -- [0, n) hi = rne(w), what
// pack_weights_kernel<__bf16> writes, and [n, 2n) lo = rne(w - hi)
__global__ void __launch_bounds__(WG)
pack_weights_split_kernel(int cin, int cout, const float* __restrict__ w, __bf16* __restrict__ fwd, __bf16* __restrict__ bwd)
{
    const int idx = blockIdx.x * WG + threadIdx.x, n = cout * cin * 9;
    if (idx >= n) return;
    const int tap = idx % 9, i = (idx / 9) % cin, o = idx / (9 * cin);
    __bf16 hi, lo;
    split_bf16(w[idx], hi, lo);
    const size_t f = ((size_t)o * 9 + tap) * cin + i, b = ((size_t)i * 9 + (8 - tap)) * cout + o;
    fwd[f] = hi; fwd[n + f] = lo;
    bwd[b] = hi; bwd[n + b] = lo;
}

// ---- conv 1_1 --------------------------------------------------------------------------------------------------------------------------
// Two threads per output row, 32 channels each.  x, y: (3,FH,FW) planes; the crop (H,W) starts at crop_origin.  (DYN a template
// parameter for the same reason as conv3x3_mfma_kernel's.)
template <bool DYN>
__global__ void __launch_bounds__(WG)
conv_first_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ rect, int FH, int FW, int H, int W,
                  const float* __restrict__ wf, const float* __restrict__ bias, const float* __restrict__ shift,
                  const float* __restrict__ scale, float* __restrict__ out, uint32_t* __restrict__ mask, const Dyn dyn)
{
    __shared__ __attribute__((aligned(16))) float s_w[27 * 64];          // [k = tap * 3 + c][channel]
    if (DYN) {
        actual_size(dyn, H, W);
        if ((int)blockIdx.x * (WG / 2) >= 2 * H * W) return;             // (the whole workgroup, before its first barrier)
    }
    for (int i = threadIdx.x; i < 27 * 64; i += WG) s_w[(i % 27) * 64 + i / 27] = wf[i];
    __syncthreads();
    const int HW = H * W;
    const int t = blockIdx.x * WG + threadIdx.x, m = t >> 1, g = t & 1;
    if (m >= 2 * HW) return;
    const int img = m >= HW, p = m - img * HW, py = p / W, px = p - py * W;
    const int2 o = crop_origin(rect, H, W, FH, FW);
    const float* src = img ? y : x;
    float in[27];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
        for (int c = 0; c < 3; c++)
            in[tap * 3 + c] = ok ? (src[((size_t)c * FH + o.y + yy) * FW + o.x + xx] - shift[c]) / scale[c] : 0.0f;
    }
    float acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = bias[32 * g + i];
#pragma unroll
    for (int k = 0; k < 27; k++) {
#pragma unroll
        for (int i = 0; i < 32; i += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(s_w + k * 64 + 32 * g + i);
            acc[i] = __fmaf_rn(in[k], wv.x, acc[i]);
            acc[i + 1] = __fmaf_rn(in[k], wv.y, acc[i + 1]);
            acc[i + 2] = __fmaf_rn(in[k], wv.z, acc[i + 2]);
            acc[i + 3] = __fmaf_rn(in[k], wv.w, acc[i + 3]);
        }
    }
    uint32_t bits = 0;
    float* dst = out + (size_t)m * 64 + 32 * g;
#pragma unroll
    for (int i = 0; i < 32; i += 4) {
        float4 v;
        v.x = fmaxf(acc[i], 0.0f); v.y = fmaxf(acc[i + 1], 0.0f); v.z = fmaxf(acc[i + 2], 0.0f); v.w = fmaxf(acc[i + 3], 0.0f);
        bits |= (uint32_t)(acc[i] > 0.0f) << i | (uint32_t)(acc[i + 1] > 0.0f) << (i + 1) | (uint32_t)(acc[i + 2] > 0.0f) << (i + 2) |
                (uint32_t)(acc[i + 3] > 0.0f) << (i + 3);
        *reinterpret_cast<float4*>(dst + i) = v;
    }
    if (mask && img == 0) mask[(size_t)m * 2 + g] = bits;
}

// The one-image form: H W rows of x alone (the forward against a reference, and -- on the ground truth, without a mask -- the reference
// pass).  A copy with the second image taken out: sharing the body moved conv_first_kernel's register allocation (92 -> 96 and 100 ->
// 120 VGPRs), and the instantiations of the two-image path are to stay the code they were.
template <bool DYN>
__global__ void __launch_bounds__(WG)
conv_first_one_kernel(const float* __restrict__ x, const int* __restrict__ rect, int FH, int FW, int H, int W,
                      const float* __restrict__ wf, const float* __restrict__ bias, const float* __restrict__ shift,
                      const float* __restrict__ scale, float* __restrict__ out, uint32_t* __restrict__ mask, const Dyn dyn)
{
    __shared__ __attribute__((aligned(16))) float s_w[27 * 64];          // [k = tap * 3 + c][channel]
    if (DYN) {
        actual_size(dyn, H, W);
        if ((int)blockIdx.x * (WG / 2) >= H * W) return;                 // (the whole workgroup, before its first barrier)
    }
    for (int i = threadIdx.x; i < 27 * 64; i += WG) s_w[(i % 27) * 64 + i / 27] = wf[i];
    __syncthreads();
    const int HW = H * W;
    const int t = blockIdx.x * WG + threadIdx.x, m = t >> 1, g = t & 1;
    if (m >= HW) return;
    const int p = m, py = p / W, px = p - py * W;
    const int2 o = crop_origin(rect, H, W, FH, FW);
    float in[27];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
        for (int c = 0; c < 3; c++)
            in[tap * 3 + c] = ok ? (x[((size_t)c * FH + o.y + yy) * FW + o.x + xx] - shift[c]) / scale[c] : 0.0f;
    }
    float acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = bias[32 * g + i];
#pragma unroll
    for (int k = 0; k < 27; k++) {
#pragma unroll
        for (int i = 0; i < 32; i += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(s_w + k * 64 + 32 * g + i);
            acc[i] = __fmaf_rn(in[k], wv.x, acc[i]);
            acc[i + 1] = __fmaf_rn(in[k], wv.y, acc[i + 1]);
            acc[i + 2] = __fmaf_rn(in[k], wv.z, acc[i + 2]);
            acc[i + 3] = __fmaf_rn(in[k], wv.w, acc[i + 3]);
        }
    }
    uint32_t bits = 0;
    float* dst = out + (size_t)m * 64 + 32 * g;
#pragma unroll
    for (int i = 0; i < 32; i += 4) {
        float4 v;
        v.x = fmaxf(acc[i], 0.0f); v.y = fmaxf(acc[i + 1], 0.0f); v.z = fmaxf(acc[i + 2], 0.0f); v.w = fmaxf(acc[i + 3], 0.0f);
        bits |= (uint32_t)(acc[i] > 0.0f) << i | (uint32_t)(acc[i + 1] > 0.0f) << (i + 1) | (uint32_t)(acc[i + 2] > 0.0f) << (i + 2) |
                (uint32_t)(acc[i + 3] > 0.0f) << (i + 3);
        *reinterpret_cast<float4*>(dst + i) = v;
    }
    if (mask) mask[(size_t)m * 2 + g] = bits;
}

// d x[c][Y][X] = g / scale[c] * sum_{tap', co} d z[q + tap'][co] wb[c][tap'][co] inside the crop, 0 outside: one thread per FRAME pixel
__global__ void __launch_bounds__(WG)
conv_first_backward_kernel(const float* __restrict__ dz, const int* __restrict__ rect, int FH, int FW, int H, int W,
                           const float* __restrict__ wb, const float* __restrict__ scale, const float* __restrict__ g_out,
                           float* __restrict__ dx, const Dyn dyn)
{
    __shared__ __attribute__((aligned(16))) float s_w[3 * 9 * 64];
    for (int i = threadIdx.x; i < 3 * 9 * 64; i += WG) s_w[i] = wb[i];
    __syncthreads();
    actual_size(dyn, H, W);
    const int t = blockIdx.x * WG + threadIdx.x;
    if (t >= FH * FW) return;
    const int Y = t / FW, X = t - Y * FW;
    const int2 o = crop_origin(rect, H, W, FH, FW);
    const int py = Y - o.y, px = X - o.x;
    const bool inside = py >= 0 && py < H && px >= 0 && px < W;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        for (int tap = 0; tap < 9; tap++) {
            const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float* row = dz + ((size_t)yy * W + xx) * 64;
#pragma unroll
            for (int co = 0; co < 64; co += 4) {
                const float4 v = *reinterpret_cast<const float4*>(row + co);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float4 wv = *reinterpret_cast<const float4*>(s_w + (c * 9 + tap) * 64 + co);
                    acc[c] = __fmaf_rn(v.x, wv.x, acc[c]);
                    acc[c] = __fmaf_rn(v.y, wv.y, acc[c]);
                    acc[c] = __fmaf_rn(v.z, wv.z, acc[c]);
                    acc[c] = __fmaf_rn(v.w, wv.w, acc[c]);
                }
            }
        }
    }
    const float g = g_out[0];
#pragma unroll
    for (int c = 0; c < 3; c++) dx[((size_t)c * FH + Y) * FW + X] = inside ? g * acc[c] / scale[c] : 0.0f;
}

// ---- the wide convolutions ---------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float* in;           // (M rows, Cin) channels-last; row m = img * H * W + y * W + x
    const float* w;            // (Cout, 9 Cin): [n][tap][ci]
    const float* bias;         // MODE_FWD
    float* out;                // (M, Cout)
    const uint32_t* mask_in;   // MODE_BWD_MASK: the sign bits of the layer this gradient arrives at, (M, Cout / 32) words
    uint32_t* mask_out;        // MODE_FWD: where this layer's sign bits go (rows < mask_rows), or null
    int M, mask_rows, H, W, Cin, Cout;
    Dyn dyn;                   // DYN: H, W are read on the device, M = nimg H W, mask_rows = H W (the fields above hold the capacity's)
    int nimg;
};

// ---- what the three wide-convolution kernels share: the size, the A tile's gather, the epilogue ----------------------------------------
// The convolution's size: the launch's, or with DYN what the device holds now.  False: every row of this workgroup lies beyond the
// actual M, and the whole workgroup returns before its first barrier.
template <bool DYN>
__device__ __forceinline__ bool conv_size(const ConvArgs& a, int m0, int& H, int& W, int& M, int& mask_rows)
{
    H = a.H; W = a.W; M = a.M; mask_rows = a.mask_rows;
    if (DYN) {
        actual_size(a.dyn, H, W);
        mask_rows = H * W;
        M = a.nimg * mask_rows;
        if (m0 >= M) return false;
    }
    return true;
}

// What one thread stages of the A tile: F4 rows, RPP apart from row `first` on, at one float4 column.  rpix: the row's index in `in`
// (-1: beyond M), ryx: its pixel as (y << 16) | x.  gather(): the four channels from `ci` on of each row's neighbour at (dy, dx), zero
// outside the image.
template <int F4, int RPP>
struct AStage {
    int rpix[F4], ryx[F4];
    __device__ __forceinline__ AStage(int first, int M, int HW, int W)
    {
#pragma unroll
        for (int i = 0; i < F4; i++) {
            const int m = first + RPP * i;
            rpix[i] = -1; ryx[i] = 0;
            if (m < M) {
                const int p = m % HW, y = p / W;
                rpix[i] = m; ryx[i] = (y << 16) | (p - y * W);
            }
        }
    }
    __device__ __forceinline__ void gather(f32x4 (&ra)[F4], const float* __restrict__ in, int H, int W, int Cin, int ci, int dy, int dx) const
    {
#pragma unroll
        for (int i = 0; i < F4; i++) {
            const int yy = (ryx[i] >> 16) + dy, xx = (ryx[i] & 0xffff) + dx;
            const bool ok = rpix[i] >= 0 && yy >= 0 && yy < H && xx >= 0 && xx < W;
            ra[i] = ok ? *reinterpret_cast<const f32x4*>(in + (size_t)(rpix[i] + dy * W + dx) * Cin + ci) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
};

// What follows the K loop (the C/D layout of the 32 x 32 tile does not depend on the operand type): bias and ReLU with the sign bits by
// one ballot per accumulator register, or the ReLU bits of the layer below, or nothing; with WK == 4 the four waves' partial blocks go
// through `s_part` (4096 floats of LDS every wave is done reading) and are summed in wave order.
template <int WK, int MODE>
__device__ __forceinline__ void conv_epilogue(const f32x16& acc0, const f32x16& acc1, float* s_part, int tid, int wave, int j, int half,
                                              int m0, int n0, int M, int mask_rows, int Cout, const float* __restrict__ bias,
                                              float* __restrict__ out, const uint32_t* __restrict__ mask_in,
                                              uint32_t* __restrict__ mask_out)
{
    // one output element per lane and call; every lane of the wave calls it (the ballot): row m, channel n = 32-aligned base + j
    auto emit = [&](float v, int m, int n) __attribute__((always_inline)) {
        const bool valid = m < M;
        if (MODE == MODE_FWD) {
            v += bias[n];
            const bool pos = v > 0.0f;
            if (valid) out[(size_t)m * Cout + n] = pos ? v : 0.0f;
            if (mask_out) {
                const unsigned long long b = __ballot(pos);
                if (j == 0 && m < mask_rows) mask_out[(size_t)m * (Cout >> 5) + (n >> 5)] = (uint32_t)(half ? b >> 32 : b);
            }
        } else if (MODE == MODE_BWD_MASK) {
            if (valid) {
                const uint32_t word = mask_in[(size_t)m * (Cout >> 5) + (n >> 5)];
                out[(size_t)m * Cout + n] = (word >> j) & 1u ? v : 0.0f;
            }
        } else {
            if (valid) out[(size_t)m * Cout + n] = v;
        }
    };
    if (WK == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) emit(acc0[r], m0 + 32 * wave + acc_row(r, half), n0 + j);
#pragma unroll
        for (int r = 0; r < 16; r++) emit(acc1[r], m0 + 32 * wave + acc_row(r, half), n0 + 32 + j);
    } else {
        // the four partial 32 x 32 blocks through LDS (s_part: every wave is past its last read), summed in wave order
#pragma unroll
        for (int b = 0; b < 2; b++) {
#pragma unroll
            for (int r = 0; r < 16; r++) s_part[wave * 1024 + acc_row(r, half) * 32 + j] = b ? acc1[r] : acc0[r];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = (tid >> 5) + 8 * i;                      // (tid >> 5) & 1 == half, tid & 31 == j
                const float* q = s_part + row * 32 + j;
                emit(((q[0] + q[1024]) + q[2048]) + q[3072], m0 + row, n0 + 32 * b + j);
            }
            __syncthreads();
        }
    }
}

// WM waves along the rows, WK waves along K (WM * WK = 4).  DYN is a template parameter so that the static instantiation stays the
// code it was.
template <int WM, int WK, int MODE, bool DYN>
__global__ void __launch_bounds__(WG)
conv3x3_mfma_kernel(const ConvArgs a)
{
    static_assert(WM * WK == 4 && (WK == 1 || WM == 1), "four waves");
    constexpr int BM = 32 * WM, A_F4 = BM * (KC / 4) / WG, B_F4 = BN * (KC / 4) / WG;
    __shared__ __attribute__((aligned(16))) float s_A[BM * LD], s_B[BN * LD];
    static_assert(BN * LD >= 4 * 32 * 32, "s_B doubles as the buffer of the four partial blocks");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    int H, W, M, mask_rows;
    if (!conv_size<DYN>(a, m0, H, W, M, mask_rows)) return;
    const int HW = H * W, Cin = a.Cin, Cout = a.Cout;
    const int K9 = 9 * Cin, nchunks = K9 / KC;
    const float* __restrict__ in = a.in;                                 // (locals: the lambdas below must not take the address of `a`)
    const float* __restrict__ bias = a.bias;
    float* __restrict__ out = a.out;
    const uint32_t* __restrict__ mask_in = a.mask_in;
    uint32_t* __restrict__ mask_out = a.mask_out;

    // the rows and float4 columns this thread stages: rows r0 + 16 i, column c4
    const int c4 = tid & 15, r0 = tid >> 4;
    const AStage<A_F4, 16> stage(m0 + r0, M, HW, W);
    const float* wbase = a.w + (size_t)(n0 + r0) * K9 + 4 * c4;
    f32x4 ra[A_F4], rb[B_F4];
    auto gload = [&](int kc) __attribute__((always_inline)) {
        const int k0 = kc * KC, tap = k0 / Cin, ci0 = k0 - tap * Cin, dy = tap / 3 - 1, dx = tap % 3 - 1;
        stage.gather(ra, in, H, W, Cin, ci0 + 4 * c4, dy, dx);
#pragma unroll
        for (int i = 0; i < B_F4; i++) rb[i] = *reinterpret_cast<const f32x4*>(wbase + (size_t)(16 * i) * K9 + k0);
    };
    auto sstore = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < A_F4; i++) *reinterpret_cast<f32x4*>(s_A + (r0 + 16 * i) * LD + 4 * c4) = ra[i];
#pragma unroll
        for (int i = 0; i < B_F4; i++) *reinterpret_cast<f32x4*>(s_B + (r0 + 16 * i) * LD + 4 * c4) = rb[i];
    };

    f32x16 acc0 = splat(0.0f), acc1 = splat(0.0f);
    const float* a_row = s_A + ((WK == 1 ? 32 * wave : 0) + j) * LD + 4 * half;
    const float* b_row = s_B + j * LD + 4 * half;
    gload(0);
    sstore();
    __syncthreads();
    for (int kc = 0; kc < nchunks; kc++) {
        if (kc + 1 < nchunks) gload(kc + 1);                             // in flight during the MFMAs of this slice
#pragma unroll
        for (int step = (WK == 1 ? 0 : wave); step < KC / 8; step += WK) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a_row + 8 * step);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_row + 8 * step);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(b_row + 32 * LD + 8 * step);
            mfma4(acc0, av, b0);
            mfma4(acc1, av, b1);
        }
        __syncthreads();
        if (kc + 1 < nchunks) {
            sstore();
            __syncthreads();
        }
    }

    conv_epilogue<WK, MODE>(acc0, acc1, s_B, tid, wave, j, half, m0, n0, M, mask_rows, Cout, bias, out, mask_in, mask_out);
}

// ---- the wide convolutions, bf16 operands ------------------------------------------------------------------------------------------
// The same implicit GEMM with both operands rounded to bf16 (nearest even) and the sums in float32, on v_mfma_f32_32x32x16_bf16: sixteen
// k per instruction at sixteen times the f32 tile's rate, so the kernel is bound by staging and is shaped for that.  The activations
// stay float32 in memory and are rounded on their way into LDS; a.w is the bf16 packing (pack_weights_kernel<__bf16>: rounded once).
// A slice is KCB channels of one tap: 128 where Cin allows (a row of 272 bytes with its padding, the f32 kernel's), 64 for the Cin =
// 64 layers and the 128-row shape (144 bytes); both strides are an odd number of 16-byte slots, so the 16-byte fragment reads of
// consecutive rows fall on different bank groups.  LDS holds TWO slices: the next one is written while this one is read, which
// leaves one barrier per slice where the f32 kernel has two.  Shapes, modes, DYN and the epilogue are the f32 kernel's.
template <int WM, int WK, int KCB, int MODE, bool DYN>
__global__ void __launch_bounds__(WG)
conv3x3_bf16_kernel(const ConvArgs a)
{
    static_assert(WM * WK == 4 && (WK == 1 || WM == 1), "four waves");
    static_assert(KCB == 64 || KCB == 128, "a slice is 64 or 128 channels");
    constexpr int BM = 32 * WM, LDB = KCB + 8, SLICE = (BM + BN) * LDB;                 // LDS row stride and one slice, in bf16
    constexpr int A_CPR = KCB / 4, A_RPP = WG / A_CPR, A_F4 = BM / A_RPP;               // A: float4 columns per row, rows per pass, passes
    constexpr int B_CPR = KCB / 8, B_RPP = WG / B_CPR, B_V8 = BN / B_RPP;               // B: the same in 8-vectors of bf16
    static_assert(KCB / 16 >= WK, "every wave has a k step in every slice");
    __shared__ __attribute__((aligned(16))) __bf16 s_ab[2 * SLICE];
    static_assert(2 * SLICE * sizeof(__bf16) >= 4 * 32 * 32 * sizeof(float), "s_ab doubles as the buffer of the four partial blocks");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    int H, W, M, mask_rows;
    if (!conv_size<DYN>(a, m0, H, W, M, mask_rows)) return;
    const int HW = H * W, Cin = a.Cin, Cout = a.Cout;
    const int K9 = 9 * Cin, nchunks = K9 / KCB;
    const float* __restrict__ in = a.in;

    // what this thread stages: of A the rows ar + A_RPP i at float4 column ac, of B the rows br + B_RPP i at 8-vector column bc
    const int ac = tid % A_CPR, ar = tid / A_CPR, bc = tid % B_CPR, br = tid / B_CPR;
    const AStage<A_F4, A_RPP> stage(m0 + ar, M, HW, W);
    const __bf16* wbase = reinterpret_cast<const __bf16*>(a.w) + (size_t)(n0 + br) * K9 + 8 * bc;
    f32x4 ra[A_F4];
    bf16x8 rb[B_V8];
    auto gload = [&](int kc) __attribute__((always_inline)) {
        const int k0 = kc * KCB, tap = k0 / Cin, ci0 = k0 - tap * Cin, dy = tap / 3 - 1, dx = tap % 3 - 1;
        stage.gather(ra, in, H, W, Cin, ci0 + 4 * ac, dy, dx);
#pragma unroll
        for (int i = 0; i < B_V8; i++) rb[i] = *reinterpret_cast<const bf16x8*>(wbase + (size_t)(B_RPP * i) * K9 + k0);
    };
    auto sstore = [&](int buf) __attribute__((always_inline)) {
        __bf16* s_A = s_ab + buf * SLICE;
        __bf16* s_B = s_A + BM * LDB;
#pragma unroll
        for (int i = 0; i < A_F4; i++) *reinterpret_cast<bf16x4*>(s_A + (ar + A_RPP * i) * LDB + 4 * ac) = to_bf16x4(ra[i]);
#pragma unroll
        for (int i = 0; i < B_V8; i++) *reinterpret_cast<bf16x8*>(s_B + (br + B_RPP * i) * LDB + 8 * bc) = rb[i];
    };

    f32x16 acc0 = splat(0.0f), acc1 = splat(0.0f);
    const int a_off = ((WK == 1 ? 32 * wave : 0) + j) * LDB + 8 * half, b_off = (BM + j) * LDB + 8 * half;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; kc++) {
        const bool more = kc + 1 < nchunks;
        if (more) gload(kc + 1);                                         // in flight during the MFMAs of this slice
        const __bf16* s = s_ab + (kc & 1) * SLICE;
#pragma unroll
        for (int step = (WK == 1 ? 0 : wave); step < KCB / 16; step += WK) {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(s + a_off + 16 * step);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(s + b_off + 16 * step);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(s + b_off + 32 * LDB + 16 * step);
            mfma16(acc0, av, b0);
            mfma16(acc1, av, b1);
        }
        if (more) sstore((kc + 1) & 1);                                  // (the other slice: every wave left it at the last barrier)
        __syncthreads();
    }
    conv_epilogue<WK, MODE>(acc0, acc1, reinterpret_cast<float*>(s_ab), tid, wave, j, half, m0, n0, M, mask_rows, Cout, a.bias, a.out, a.mask_in, a.mask_out);
}

// ---- the wide convolutions, split-bf16 operands (three products) ---------------------------------------------------------------------
// The same implicit GEMM with every float32 operand a carried as two bf16, hi(a) = rne(a) and lo(a) = rne(a - hi(a)) (split_bf16,
// mfma_bf16.h), and every product a b replaced by
//     lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)
// on v_mfma_f32_32x32x16_bf16: three exact bf16 x bf16 products summed in float32, lo(a) lo(b) dropped.  A single product is off by at
// most 2^-15 |a b| (|a - hi - lo| <= 2^-17 |a| for either operand, the dropped product at most 2^-16 |a b|); the sums are held to
// 2^-16 of mass = conv(|in|, |w|) + |bias| per element by the tests and measure 0.04-0.12 of it.  A lo below bf16's normal range
// (|lo| < 2^-126) may be flushed by the matrix core: not part of the contract.  It equals ONE plain convolution over 3 Cin channels,
// inputs [lo, hi, hi] against weights [hi, lo, hi].
//   The activations (forward) and incoming gradients (backward) stay float32 in memory and are split by the staging thread on their
// way into LDS; a.w is the split packing (pack_weights_split_kernel: a hi plane, which is the bf16 packing, and a lo plane of the same
// layout Cout * 9 Cin values further on).  A slice is KCB channels of one tap in FOUR planes (A hi, A lo, B hi, B lo), rows of KCB + 8
// bf16 as in conv3x3_bf16_kernel: the float32 kernel's bytes.  LDS holds ONE slice, with the f32 kernel's two barriers around its
// refill: 55 296 bytes in the 128-row shape (two workgroups per CU), 52 224 / 27 648 in the 32-row shape with 128 / 64 channels.  A
// second slice (one barrier) was measured in every shape and lost or changed nothing: it costs workgroups per CU, which hide more.
//   The order, per k step of sixteen: small += lo(a) hi(b); acc += hi(a) hi(b); small += hi(a) lo(b) -- the two small terms in an
// accumulator pair of their own, added to the large one element by element once, after the last slice.  Four independent chains
// instead of two: the same MFMAs into ONE pair were 20 % slower at 256 x 176 (each waits for the one before it); the 32 registers
// more cost no occupancy.  The 32-row shape asks for three waves per SIMD (it is launched when the grid is small, and its 180
// registers would otherwise leave two).  Shapes, modes, DYN and the epilogue are conv3x3_bf16_kernel's.  profiles/lpips_notes.md.
template <int WM, int WK, int KCB, int MODE, bool DYN>
__global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(WK == 4 ? 3 : 2)))
conv3x3_bf16x3_kernel(const ConvArgs a)
{
    static_assert(WM * WK == 4 && (WK == 1 || WM == 1), "four waves");
    static_assert(KCB == 64 || KCB == 128, "a slice is 64 or 128 channels");
    constexpr int BM = 32 * WM, LDB = KCB + 8;                                          // LDS row stride, in bf16
    constexpr int A_LO = BM * LDB, B_HI = 2 * BM * LDB, B_LO = B_HI + BN * LDB, SLICE = 2 * (BM + BN) * LDB;   // the planes of a slice
    constexpr int A_CPR = KCB / 4, A_RPP = WG / A_CPR, A_F4 = BM / A_RPP;               // A: float4 columns per row, rows per pass, passes
    constexpr int B_CPR = KCB / 8, B_RPP = WG / B_CPR, B_V8 = BN / B_RPP;               // B: the same in 8-vectors of bf16, per plane
    static_assert(KCB / 16 >= WK, "every wave has a k step in every slice");
    __shared__ __attribute__((aligned(16))) __bf16 s_ab[SLICE];
    static_assert(SLICE * sizeof(__bf16) >= 4 * 32 * 32 * sizeof(float), "s_ab doubles as the buffer of the four partial blocks");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    int H, W, M, mask_rows;
    if (!conv_size<DYN>(a, m0, H, W, M, mask_rows)) return;
    const int HW = H * W, Cin = a.Cin, Cout = a.Cout;
    const int K9 = 9 * Cin, nchunks = K9 / KCB;
    const float* __restrict__ in = a.in;

    // what this thread stages: of A the rows ar + A_RPP i at float4 column ac, of B (both planes) the rows br + B_RPP i at 8-vector column bc
    const int ac = tid % A_CPR, ar = tid / A_CPR, bc = tid % B_CPR, br = tid / B_CPR;
    // AStage's table and, in gload, its gather, written out: through AStage the 128-row forward of this kernel alone was slower (512x352
    // forward 1 648 -> 1 693 us; profiles/lpips_notes.md) where the other two kernels gained, and the cause was not found
    int rpix[A_F4], ryx[A_F4];
#pragma unroll
    for (int i = 0; i < A_F4; i++) {
        const int m = m0 + ar + A_RPP * i;
        rpix[i] = -1; ryx[i] = 0;
        if (m < M) {
            const int p = m % HW, y = p / W;
            rpix[i] = m; ryx[i] = (y << 16) | (p - y * W);
        }
    }
    const __bf16* whi = reinterpret_cast<const __bf16*>(a.w) + (size_t)(n0 + br) * K9 + 8 * bc;
    const __bf16* wlo = whi + (size_t)Cout * K9;
    f32x4 ra[A_F4];
    bf16x8 rbh[B_V8], rbl[B_V8];
    auto gload = [&](int kc) __attribute__((always_inline)) {
        const int k0 = kc * KCB, tap = k0 / Cin, ci0 = k0 - tap * Cin, dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
        for (int i = 0; i < A_F4; i++) {
            const int yy = (ryx[i] >> 16) + dy, xx = (ryx[i] & 0xffff) + dx;
            const bool ok = rpix[i] >= 0 && yy >= 0 && yy < H && xx >= 0 && xx < W;
            ra[i] = ok ? *reinterpret_cast<const f32x4*>(in + (size_t)(rpix[i] + dy * W + dx) * Cin + ci0 + 4 * ac)
                       : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int i = 0; i < B_V8; i++) {
            rbh[i] = *reinterpret_cast<const bf16x8*>(whi + (size_t)(B_RPP * i) * K9 + k0);
            rbl[i] = *reinterpret_cast<const bf16x8*>(wlo + (size_t)(B_RPP * i) * K9 + k0);
        }
    };
    auto sstore = [&]() __attribute__((always_inline)) {
        __bf16* s = s_ab;
#pragma unroll
        for (int i = 0; i < A_F4; i++) {
            bf16x4 hi, lo;
            split_bf16x4(ra[i], hi, lo);
            *reinterpret_cast<bf16x4*>(s + (ar + A_RPP * i) * LDB + 4 * ac) = hi;
            *reinterpret_cast<bf16x4*>(s + A_LO + (ar + A_RPP * i) * LDB + 4 * ac) = lo;
        }
#pragma unroll
        for (int i = 0; i < B_V8; i++) {
            *reinterpret_cast<bf16x8*>(s + B_HI + (br + B_RPP * i) * LDB + 8 * bc) = rbh[i];
            *reinterpret_cast<bf16x8*>(s + B_LO + (br + B_RPP * i) * LDB + 8 * bc) = rbl[i];
        }
    };

    f32x16 acc0 = splat(0.0f), acc1 = splat(0.0f), small0 = splat(0.0f), small1 = splat(0.0f);
    const int a_off = ((WK == 1 ? 32 * wave : 0) + j) * LDB + 8 * half, b_off = j * LDB + 8 * half;
    gload(0);
    sstore();
    __syncthreads();
    const __bf16* s = s_ab;
    for (int kc = 0; kc < nchunks; kc++) {
        const bool more = kc + 1 < nchunks;
        if (more) gload(kc + 1);                                         // in flight during the MFMAs of this slice
#pragma unroll
        for (int step = (WK == 1 ? 0 : wave); step < KCB / 16; step += WK) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(s + a_off + 16 * step);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(s + A_LO + a_off + 16 * step);
            const bf16x8 bh0 = *reinterpret_cast<const bf16x8*>(s + B_HI + b_off + 16 * step);
            const bf16x8 bh1 = *reinterpret_cast<const bf16x8*>(s + B_HI + b_off + 32 * LDB + 16 * step);
            const bf16x8 bl0 = *reinterpret_cast<const bf16x8*>(s + B_LO + b_off + 16 * step);
            const bf16x8 bl1 = *reinterpret_cast<const bf16x8*>(s + B_LO + b_off + 32 * LDB + 16 * step);
            mfma16(small0, al, bh0);
            mfma16(small1, al, bh1);
            mfma16(acc0, ah, bh0);
            mfma16(acc1, ah, bh1);
            mfma16(small0, ah, bl0);
            mfma16(small1, ah, bl1);
        }
        __syncthreads();
        if (more) {
            sstore();
            __syncthreads();
        }
    }
    acc0 += small0;                                                      // (element by element: the small terms join the large one once)
    acc1 += small1;
    conv_epilogue<WK, MODE>(acc0, acc1, reinterpret_cast<float*>(s_ab), tid, wave, j, half, m0, n0, M, mask_rows, Cout, a.bias, a.out, a.mask_in, a.mask_out);
}

// ---- 2x2 max-pool, stride 2, floor ---------------------------------------------------------------------------------------------------
// One thread per pooled row and 16 channels.  The winner (first maximum in the order (0,0) (0,1) (1,0) (1,1)), two bits per channel,
// is kept for the first image when `win` is given: (pooled row, C / 16) words.
__global__ void __launch_bounds__(WG)
pool_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t* __restrict__ win, int nimg, int H, int W, int C,
            const Dyn dyn)
{
    actual_size(dyn, H, W);
    const int Hp = H >> 1, Wp = W >> 1, G = C >> 4;
    const long long t = (long long)blockIdx.x * WG + threadIdx.x;
    if (t >= (long long)nimg * Hp * Wp * G) return;
    const int g = (int)(t % G);
    const int q = (int)(t / G), img = q / (Hp * Wp), pp = q - img * (Hp * Wp), py = pp / Wp, px = pp - py * Wp;
    const float* base = in + (((size_t)img * H + 2 * py) * W + 2 * px) * C + 16 * g;
    float* dst = out + (size_t)q * C + 16 * g;
    uint32_t word = 0;
#pragma unroll
    for (int quad = 0; quad < 4; quad++) {
        const float4 v0 = *reinterpret_cast<const float4*>(base + 4 * quad);
        const float4 v1 = *reinterpret_cast<const float4*>(base + C + 4 * quad);
        const float4 v2 = *reinterpret_cast<const float4*>(base + (size_t)W * C + 4 * quad);
        const float4 v3 = *reinterpret_cast<const float4*>(base + (size_t)W * C + C + 4 * quad);
        const float c0[4] = {v0.x, v0.y, v0.z, v0.w}, c1[4] = {v1.x, v1.y, v1.z, v1.w}, c2[4] = {v2.x, v2.y, v2.z, v2.w},
                    c3[4] = {v3.x, v3.y, v3.z, v3.w};
        float best[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            uint32_t idx = 0;
            best[e] = c0[e];
            if (c1[e] > best[e]) { best[e] = c1[e]; idx = 1; }
            if (c2[e] > best[e]) { best[e] = c2[e]; idx = 2; }
            if (c3[e] > best[e]) { best[e] = c3[e]; idx = 3; }
            word |= idx << (2 * (4 * quad + e));
        }
        *reinterpret_cast<float4*>(dst + 4 * quad) = make_float4(best[0], best[1], best[2], best[3]);
    }
    if (win && img == 0) win[(size_t)pp * G + g] = word;
}

// ---- a tap: one wave per pixel ---------------------------------------------------------------------------------------------------------
// f: the tapped activations of both images ((2, HW, C): y's follow x's).  partial[p] = sum_c lin[c] (nx - ny)^2; with G also
// G[p][c] = d term / d fx[p][c] for term = mean_p partial[p]:  a = 2 lin (nx - ny) / HW,  G = a / (s + eps) - fx (a . fx) / (s (s + eps)^2).
__global__ void __launch_bounds__(WG)
tap_kernel(const float* __restrict__ f, int HW, int C, const float* __restrict__ lin, float* __restrict__ partial, float* __restrict__ G,
           const Dyn dyn)
{
    if (dyn.cap_H > 0) {
        int H = 0, W = 0;
        actual_size(dyn, H, W);
        HW = H * W;
    }
    const int lane = threadIdx.x & 63, p = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (p >= HW) return;
    const int n = C >> 6;
    const float* rx = f + (size_t)p * C + lane;
    const float* ry = rx + (size_t)HW * C;
    float fx[8], fy[8], w[8], sx2 = 0.0f, sy2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        fx[i] = fy[i] = w[i] = 0.0f;
        if (i < n) {
            fx[i] = rx[64 * i]; fy[i] = ry[64 * i]; w[i] = lin[lane + 64 * i];
            sx2 = __fmaf_rn(fx[i], fx[i], sx2);
            sy2 = __fmaf_rn(fy[i], fy[i], sy2);
        }
    }
    const float sx = sqrtf(wave_sum(sx2)), sy = sqrtf(wave_sum(sy2)), ex = sx + NORM_EPS, ey = sy + NORM_EPS;
    float av[8], t = 0.0f, dot = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        av[i] = 0.0f;
        if (i < n) {
            const float d = fx[i] / ex - fy[i] / ey;
            t = __fmaf_rn(w[i] * d, d, t);
            av[i] = 2.0f * w[i] * d / (float)HW;
            dot = __fmaf_rn(av[i], fx[i], dot);
        }
    }
    t = wave_sum(t);
    if (lane == 0) partial[p] = t;
    if (G) {
        dot = wave_sum(dot);
        const float k = sx > 0.0f ? dot / (sx * ex * ex) : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i < n) G[(size_t)p * C + lane + 64 * i] = av[i] / ex - fx[i] * k;
    }
}

// The tap of the forward against a reference: f holds x's activations alone and y's row comes from `fyref`, a region of a reference
// block (HW rows of C, the same layout) -- the same float32 operations on the same values.  A copy with that one line changed:
// sharing the body moved tap_kernel's scalar prologue, and the kernels of the two-image path are to stay the code they were.
__global__ void __launch_bounds__(WG)
tap_ref_kernel(const float* __restrict__ f, const float* __restrict__ fyref, int HW, int C, const float* __restrict__ lin,
               float* __restrict__ partial, float* __restrict__ G, const Dyn dyn)
{
    if (dyn.cap_H > 0) {
        int H = 0, W = 0;
        actual_size(dyn, H, W);
        HW = H * W;
    }
    const int lane = threadIdx.x & 63, p = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (p >= HW) return;
    const int n = C >> 6;
    const float* rx = f + (size_t)p * C + lane;
    const float* ry = fyref + (size_t)p * C + lane;
    float fx[8], fy[8], w[8], sx2 = 0.0f, sy2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        fx[i] = fy[i] = w[i] = 0.0f;
        if (i < n) {
            fx[i] = rx[64 * i]; fy[i] = ry[64 * i]; w[i] = lin[lane + 64 * i];
            sx2 = __fmaf_rn(fx[i], fx[i], sx2);
            sy2 = __fmaf_rn(fy[i], fy[i], sy2);
        }
    }
    const float sx = sqrtf(wave_sum(sx2)), sy = sqrtf(wave_sum(sy2)), ex = sx + NORM_EPS, ey = sy + NORM_EPS;
    float av[8], t = 0.0f, dot = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        av[i] = 0.0f;
        if (i < n) {
            const float d = fx[i] / ex - fy[i] / ey;
            t = __fmaf_rn(w[i] * d, d, t);
            av[i] = 2.0f * w[i] * d / (float)HW;
            dot = __fmaf_rn(av[i], fx[i], dot);
        }
    }
    t = wave_sum(t);
    if (lane == 0) partial[p] = t;
    if (G) {
        dot = wave_sum(dot);
        const float k = sx > 0.0f ? dot / (sx * ex * ex) : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i < n) G[(size_t)p * C + lane + 64 * i] = av[i] / ex - fx[i] * k;
    }
}

struct ReduceArgs {
    int off[NTAP], cnt[NTAP];
    Dyn dyn;                   // with a capacity cnt[l] is (h >> l) * (w >> l) of the device rectangle
};

// the five spatial means and their sum: one workgroup, float64 sums in a fixed order
__global__ void __launch_bounds__(1024)
reduce_kernel(const float* __restrict__ partial, const ReduceArgs r, float* __restrict__ out, float* __restrict__ terms)
{
    __shared__ double s[1024];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int l = 0; l < NTAP; l++) {
        int cnt = r.cnt[l];
        if (r.dyn.cap_H > 0) {
            int H = 0, W = 0;
            actual_size(r.dyn, H, W);
            cnt = (H >> l) * (W >> l);
        }
        double v = 0.0;
        for (int p = tid; p < cnt; p += 1024) v += (double)partial[r.off[l] + p];
        s[tid] = v;
        __syncthreads();
        for (int st = 512; st > 0; st >>= 1) {
            if (tid < st) s[tid] += s[tid + st];
            __syncthreads();
        }
        const double term = s[0] / (double)cnt;
        if (tid == 0 && terms) terms[l] = (float)term;
        total += term;
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)total;
}

// ---- backward through a tap and the pool above it -----------------------------------------------------------------------------------
// d z[p][c] = relu bit ? G[p][c] + (the pooled gradient where (p, c) won its 2x2 window) : 0.  One thread per row and 4 channels.
// dpool null: the last tap, nothing comes from above.
__global__ void __launch_bounds__(WG)
unpool_tap_kernel(const float* __restrict__ G, const float* __restrict__ dpool, const uint32_t* __restrict__ win,
                  const uint32_t* __restrict__ mask, float* __restrict__ out, int H, int W, int C, const Dyn dyn)
{
    actual_size(dyn, H, W);
    const int Q = C >> 2;
    const long long t = (long long)blockIdx.x * WG + threadIdx.x;
    if (t >= (long long)H * W * Q) return;
    const int c = 4 * (int)(t % Q), p = (int)(t / Q), y = p / W, x = p - y * W;
    const float4 g = *reinterpret_cast<const float4*>(G + (size_t)p * C + c);
    float v[4] = {g.x, g.y, g.z, g.w};
    const int Hp = H >> 1, Wp = W >> 1;
    if (dpool && (y >> 1) < Hp && (x >> 1) < Wp) {
        const int pp = (y >> 1) * Wp + (x >> 1);
        const uint32_t pos = (uint32_t)((y & 1) * 2 + (x & 1));
        const uint32_t word = win[(size_t)pp * (C >> 4) + (c >> 4)] >> (2 * (c & 15));
        const float4 d = *reinterpret_cast<const float4*>(dpool + (size_t)pp * C + c);
        const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (((word >> (2 * e)) & 3u) == pos) v[e] += dv[e];
    }
    const uint32_t bits = mask[(size_t)p * (C >> 5) + (c >> 5)] >> (c & 31);
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (!((bits >> e) & 1u)) v[e] = 0.0f;
    *reinterpret_cast<float4*>(out + (size_t)p * C + c) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct Geo {
    int H[NTAP], W[NTAP];
    size_t mask_off[NCONV], win_off[NTAP - 1], g_off[NTAP], saved_bytes;          // byte offsets into `saved`
    size_t buf_bytes, partial_off[NTAP], workspace_bytes;                           // partial_off: floats into the partial array
    size_t ref_off[NTAP], reference_bytes;                                          // byte offsets into a reference block
};

Geo geometry(int H, int W)
{
    Geo g{};
    for (int l = 0; l < NTAP; l++) { g.H[l] = H >> l; g.W[l] = W >> l; }
    size_t off = 0;
    for (int i = 0; i < NCONV; i++) {
        const int l = CONV_LEVEL[i];
        g.mask_off[i] = off;
        off += align_up((size_t)g.H[l] * g.W[l] * (CONV_COUT[i] / 32) * sizeof(uint32_t));
    }
    for (int l = 0; l + 1 < NTAP; l++) {
        g.win_off[l] = off;
        off += align_up((size_t)g.H[l + 1] * g.W[l + 1] * (TAP_C[l] / 16) * sizeof(uint32_t));
    }
    for (int l = 0; l < NTAP; l++) {
        g.g_off[l] = off;
        off += align_up((size_t)g.H[l] * g.W[l] * TAP_C[l] * sizeof(float));
    }
    g.saved_bytes = off;
    g.buf_bytes = align_up((size_t)2 * H * W * 64 * sizeof(float));                // the largest activation: 64 channels at full size, two images
    size_t n = 0;
    for (int l = 0; l < NTAP; l++) { g.partial_off[l] = n; n += (size_t)g.H[l] * g.W[l]; }
    g.workspace_bytes = 2 * g.buf_bytes + align_up(n * sizeof(float));
    off = 0;
    for (int l = 0; l < NTAP; l++) {                                               // the tapped activations of ONE image
        g.ref_off[l] = off;
        off += align_up((size_t)g.H[l] * g.W[l] * TAP_C[l] * sizeof(float));
    }
    g.reference_bytes = off;
    return g;
}

// The conv kernels pack a row's pixel as (y << 16) | x in an int and take x = packed & 0xffff, y = packed >> 16: x <= 65535 and
// y <= 32767 (one more and the shift reaches the sign bit), that is W <= 65536 and H <= 32768.
constexpr int MAX_H = 1 << 15, MAX_W = 1 << 16;
bool packing_ok(int H, int W) { return H <= MAX_H && W <= MAX_W; }

// (32-bit element indices: 2 H W 64 < 2^31)
bool size_ok(int H, int W) { return H >= 16 && W >= 16 && (long long)H * W <= (1ll << 22) && packing_ok(H, W); }

// which of the two kernel shapes a wide convolution takes: the launcher's own choice, or the caller's (moss_lpips_vgg_conv3x3)
enum { SHAPE_AUTO, SHAPE_ROWS128, SHAPE_ROWS32 };

// the 128-row shape where its grid fills the device, the 32-row split-K shape for the deep layers' few rows
inline bool rows128(const ConvArgs& a, int shape)
{
    return shape == SHAPE_AUTO ? (a.M + 127) / 128 * (a.Cout / BN) >= device_cus() : shape == SHAPE_ROWS128;
}

// a.M: the rows the grid covers and the shape is picked by -- with a capacity the capacity's, whatever the crop turns out to be
template <int MODE, bool DYN>
void launch_conv_as(const ConvArgs& a, int shape, hipStream_t s)
{
    if (rows128(a, shape))
        hipLaunchKernelGGL((conv3x3_mfma_kernel<4, 1, MODE, DYN>), dim3((a.M + 127) / 128, a.Cout / BN), dim3(WG), 0, s, a);
    else
        hipLaunchKernelGGL((conv3x3_mfma_kernel<1, 4, MODE, DYN>), dim3((a.M + 31) / 32, a.Cout / BN), dim3(WG), 0, s, a);
}

// the same choice of shape for the bf16 kernel; a slice of 128 channels where Cin has them and the shape has the LDS for two
template <int MODE, bool DYN>
void launch_conv_bf16_as(const ConvArgs& a, int shape, hipStream_t s)
{
    if (rows128(a, shape))
        hipLaunchKernelGGL((conv3x3_bf16_kernel<4, 1, 64, MODE, DYN>), dim3((a.M + 127) / 128, a.Cout / BN), dim3(WG), 0, s, a);
    else if (a.Cin % 128 == 0)
        hipLaunchKernelGGL((conv3x3_bf16_kernel<1, 4, 128, MODE, DYN>), dim3((a.M + 31) / 32, a.Cout / BN), dim3(WG), 0, s, a);
    else
        hipLaunchKernelGGL((conv3x3_bf16_kernel<1, 4, 64, MODE, DYN>), dim3((a.M + 31) / 32, a.Cout / BN), dim3(WG), 0, s, a);
}

// the same choice of shape for the split-bf16 kernel, and the bf16 kernel's choice of slice: 64 channels in the 128-row shape, 128 in
// the 32-row shape where Cin has them (two k steps per wave and barrier pair instead of one: 17 % faster at 256 x 176)
template <int MODE, bool DYN>
void launch_conv_bf16x3_as(const ConvArgs& a, int shape, hipStream_t s)
{
    if (rows128(a, shape))
        hipLaunchKernelGGL((conv3x3_bf16x3_kernel<4, 1, 64, MODE, DYN>), dim3((a.M + 127) / 128, a.Cout / BN), dim3(WG), 0, s, a);
    else if (a.Cin % 128 == 0)
        hipLaunchKernelGGL((conv3x3_bf16x3_kernel<1, 4, 128, MODE, DYN>), dim3((a.M + 31) / 32, a.Cout / BN), dim3(WG), 0, s, a);
    else
        hipLaunchKernelGGL((conv3x3_bf16x3_kernel<1, 4, 64, MODE, DYN>), dim3((a.M + 31) / 32, a.Cout / BN), dim3(WG), 0, s, a);
}

// the operands of the wide convolutions.  PREC_BF16: a.w is the bf16 packing and the operands are rounded (conv3x3_bf16_kernel);
// PREC_BF16X3: a.w is the split packing and every product is three (conv3x3_bf16x3_kernel)
enum Precision { PREC_F32, PREC_BF16, PREC_BF16X3 };

template <int MODE>
void launch_conv(const ConvArgs& a, Precision prec, hipStream_t s, int shape = SHAPE_AUTO)
{
    if (prec == PREC_BF16X3) {
        if (a.dyn.cap_H > 0) launch_conv_bf16x3_as<MODE, true>(a, shape, s); else launch_conv_bf16x3_as<MODE, false>(a, shape, s);
    } else if (prec == PREC_BF16) {
        if (a.dyn.cap_H > 0) launch_conv_bf16_as<MODE, true>(a, shape, s); else launch_conv_bf16_as<MODE, false>(a, shape, s);
    } else {
        if (a.dyn.cap_H > 0) launch_conv_as<MODE, true>(a, shape, s); else launch_conv_as<MODE, false>(a, shape, s);
    }
}

int grid_for(long long threads) { return (int)((threads + WG - 1) / WG); }

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_lpips_vgg_workspace_bytes(int H, int W) { return size_ok(H, W) ? geometry(H, W).workspace_bytes : 0; }

extern "C" size_t moss_lpips_vgg_saved_bytes(int H, int W) { return size_ok(H, W) ? geometry(H, W).saved_bytes : 0; }

extern "C" int moss_lpips_vgg_pack_weights(int cin, int cout, const float* w, float* fwd, float* bwd, void* stream)
{
    if (cin <= 0 || cout <= 0 || !w || !fwd || !bwd) return invalid_arg("moss_lpips_vgg_pack_weights", "sizes <= 0 or a null pointer");
    hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(grid_for((long long)cin * cout * 9)), dim3(WG), 0, (hipStream_t)stream, cin, cout, w, fwd, bwd);
    return launch_status("moss_lpips_vgg_pack_weights");
}

extern "C" int moss_lpips_vgg_pack_weights_bf16(int cin, int cout, const float* w, uint16_t* fwd, uint16_t* bwd, void* stream)
{
    const char* me = "moss_lpips_vgg_pack_weights_bf16";
    if (cin <= 0 || cout <= 0 || !w || !fwd || !bwd) return invalid_arg(me, "sizes <= 0 or a null pointer");
    hipLaunchKernelGGL(pack_weights_kernel<__bf16>, dim3(grid_for((long long)cin * cout * 9)), dim3(WG), 0, (hipStream_t)stream, cin, cout, w,
                       reinterpret_cast<__bf16*>(fwd), reinterpret_cast<__bf16*>(bwd));
    return launch_status(me);
}

extern "C" int moss_lpips_vgg_pack_weights_bf16x3(int cin, int cout, const float* w, uint16_t* fwd, uint16_t* bwd, void* stream)
{
    const char* me = "moss_lpips_vgg_pack_weights_bf16x3";
    if (cin <= 0 || cout <= 0 || !w || !fwd || !bwd) return invalid_arg(me, "sizes <= 0 or a null pointer");
    hipLaunchKernelGGL(pack_weights_split_kernel, dim3(grid_for((long long)cin * cout * 9)), dim3(WG), 0, (hipStream_t)stream, cin, cout, w,
                       reinterpret_cast<__bf16*>(fwd), reinterpret_cast<__bf16*>(bwd));
    return launch_status(me);
}

// H, W: on return the size the launches and the regions of `saved` and `workspace` are made for -- the crop's, or the capacity's
static const char* check_frame(int& H, int& W, int cap_H, int cap_W, const int* rect, int& FH, int& FW)
{
    if (cap_H || cap_W) {
        if (cap_H <= 0 || cap_W <= 0) return "cap_H and cap_W must both be set (or both 0: the static call)";
        if (!rect) return "a capacity needs rect: the crop's size is read from it on the device";
        if (!size_ok(cap_H, cap_W)) return "the capacity must be >= 16 per axis (four 2x2 pools), cap_H <= 32768, cap_W <= 65536 and cap_H * cap_W <= 2^22";
        if (FH == 0 && FW == 0) { FH = cap_H; FW = cap_W; }
        if (FH < cap_H || FW < cap_W) return "the capacity is larger than the frame";
        H = cap_H; W = cap_W;
        return nullptr;
    }
    if (!size_ok(H, W)) return "H and W must be >= 16 (four 2x2 pools), H <= 32768, W <= 65536 and H * W <= 2^22";
    if (FH == 0 && FW == 0) { FH = H; FW = W; }
    if (FH < H || FW < W) return "the frame is smaller than the crop";
    return nullptr;
}

static const char* SHORT_WORKSPACE = "the workspace is null or smaller than moss_lpips_vgg_workspace_bytes(H, W) (of cap_H, cap_W with a capacity)";

// What the three forwards share.  The two-image call: x and y, the batch of two.  The forward against a reference: x alone (nimg = 1,
// M = H W), the taps read y's activations from ref_in.  The reference pass: `x` is the ground truth, alone; the tapped layers write
// straight into their regions of ref_out, the pools read them there, and there is no tap, no mean and no `saved`.
struct FwdCall {
    const float* x;
    const float* y;                          // the two-image call, else null
    const char* ref_in;                      // the forward against a reference, else null
    char* ref_out;                           // the reference pass, else null
    const int* rect;
    int cap_H, cap_W;
    const float* const* weights;
    const float* const* biases;
    const float* const* lin;
    const float* shift;
    const float* scale;
    float* out;
    float* terms;
    char* saved;
    char* workspace;
};

// H, W: the crop's size or the capacity's (check_frame).  launch_conv picks each layer's shape from the rows THIS call has.
static void forward_launches(const FwdCall& f, const Geo& g, int H, int W, int FH, int FW, Precision prec, hipStream_t s)
{
    const int nimg = f.y ? 2 : 1;
    auto dyn_at = [&](int level) { return Dyn{f.rect, f.cap_H, f.cap_W, level}; };        // (cap_H == 0: the kernels take the sizes below)
    float* const ws[2] = {reinterpret_cast<float*>(f.workspace), reinterpret_cast<float*>(f.workspace + g.buf_bytes)};
    float* partial = reinterpret_cast<float*>(f.workspace + 2 * g.buf_bytes);
    char* sv = f.saved;
    auto mask_at = [&](int i) { return sv ? reinterpret_cast<uint32_t*>(sv + g.mask_off[i]) : nullptr; };
    auto other = [&](const float* in) { return in == ws[0] ? ws[1] : ws[0]; };             // a workspace buffer `in` is not

    const int HW0 = H * W;
    float* cur = ws[0];
    if (nimg == 2) {
        if (f.cap_H > 0)
            hipLaunchKernelGGL(conv_first_kernel<true>, dim3(grid_for(4ll * HW0)), dim3(WG), 0, s, f.x, f.y, f.rect, FH, FW, H, W,
                               f.weights[0], f.biases[0], f.shift, f.scale, cur, mask_at(0), dyn_at(0));
        else
            hipLaunchKernelGGL(conv_first_kernel<false>, dim3(grid_for(4ll * HW0)), dim3(WG), 0, s, f.x, f.y, f.rect, FH, FW, H, W,
                               f.weights[0], f.biases[0], f.shift, f.scale, cur, mask_at(0), dyn_at(0));
    } else {
        if (f.cap_H > 0)
            hipLaunchKernelGGL(conv_first_one_kernel<true>, dim3(grid_for(2ll * HW0)), dim3(WG), 0, s, f.x, f.rect, FH, FW, H, W,
                               f.weights[0], f.biases[0], f.shift, f.scale, cur, mask_at(0), dyn_at(0));
        else
            hipLaunchKernelGGL(conv_first_one_kernel<false>, dim3(grid_for(2ll * HW0)), dim3(WG), 0, s, f.x, f.rect, FH, FW, H, W,
                               f.weights[0], f.biases[0], f.shift, f.scale, cur, mask_at(0), dyn_at(0));
    }
    int tap = 0;
    ReduceArgs red{};
    red.dyn = dyn_at(0);
    for (int i = 1; i < NCONV; i++) {
        const int l = CONV_LEVEL[i], HW = g.H[l] * g.W[l];
        const bool tapped = i == TAP_CONV[tap];
        float* out = tapped && f.ref_out ? reinterpret_cast<float*>(f.ref_out + g.ref_off[tap]) : other(cur);
        ConvArgs c{};
        c.in = cur; c.w = f.weights[i]; c.bias = f.biases[i]; c.out = out; c.mask_out = mask_at(i);
        c.M = nimg * HW; c.mask_rows = HW; c.H = g.H[l]; c.W = g.W[l]; c.Cin = CONV_COUT[i - 1]; c.Cout = CONV_COUT[i];
        c.dyn = dyn_at(l); c.nimg = nimg;
        launch_conv<MODE_FWD>(c, prec, s);
        cur = out;
        if (!tapped) continue;
        const int C = TAP_C[tap];
        float* G = sv ? reinterpret_cast<float*>(sv + g.g_off[tap]) : nullptr;
        if (f.y)
            hipLaunchKernelGGL(tap_kernel, dim3((HW + 3) / 4), dim3(WG), 0, s, (const float*)cur, HW, C, f.lin[tap],
                               partial + g.partial_off[tap], G, dyn_at(l));
        else if (f.ref_in)
            hipLaunchKernelGGL(tap_ref_kernel, dim3((HW + 3) / 4), dim3(WG), 0, s, (const float*)cur,
                               reinterpret_cast<const float*>(f.ref_in + g.ref_off[tap]), HW, C, f.lin[tap], partial + g.partial_off[tap],
                               G, dyn_at(l));
        red.off[tap] = (int)g.partial_off[tap];
        red.cnt[tap] = HW;
        if (tap + 1 < NTAP) {
            out = other(cur);
            hipLaunchKernelGGL(pool_kernel, dim3(grid_for((long long)nimg * g.H[l + 1] * g.W[l + 1] * (C / 16))), dim3(WG), 0, s,
                               (const float*)cur, out, sv ? reinterpret_cast<uint32_t*>(sv + g.win_off[tap]) : nullptr, nimg, g.H[l], g.W[l],
                               C, dyn_at(l));
            cur = out;
        }
        tap++;
    }
    if (!f.ref_out) hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(1024), 0, s, (const float*)partial, red, f.out, f.terms);
}

static const char* null_weights(const float* const* weights, const float* const* biases)
{
    for (int i = 0; i < NCONV; i++)
        if (!weights[i] || !biases[i]) return "null weight or bias (13 of each, packed by moss_lpips_vgg_pack_weights)";
    return nullptr;
}

// LPIPS.forward, lpipsPyTorch/modules/lpips.py:31-37 (net_type='vgg').  prec: weights[1..12] are that precision's packing
static int lpips_forward(const char* me, const moss_lpips_vgg_args* a, Precision prec, void* stream)
{
    if (!a) return invalid_arg(me, "null argument block");
    int FH = a->frame_H, FW = a->frame_W;
    int H = a->H, W = a->W;
    if (const char* why = check_frame(H, W, a->cap_H, a->cap_W, a->rect, FH, FW)) return invalid_arg(me, why);
    if (!a->x || !a->y || !a->out || !a->shift || !a->scale) return invalid_arg(me, "null x, y, out, shift or scale");
    if (const char* why = null_weights(a->weights, a->biases)) return invalid_arg(me, why);
    for (int l = 0; l < NTAP; l++)
        if (!a->lin[l]) return invalid_arg(me, "null lin weight (5)");
    const Geo g = geometry(H, W);
    if (!a->workspace || a->workspace_bytes < g.workspace_bytes) return invalid_arg(me, SHORT_WORKSPACE);
    const FwdCall f{a->x, a->y, nullptr, nullptr, a->rect, a->cap_H, a->cap_W, a->weights, a->biases, a->lin, a->shift, a->scale,
                    a->out, a->terms, a->saved, a->workspace};
    forward_launches(f, g, H, W, FH, FW, prec, (hipStream_t)stream);
    return launch_status(me);
}

static const char* SHORT_REFERENCE = "reference is null or reference_bytes is smaller than moss_lpips_vgg_reference_bytes(H, W) (of cap_H, cap_W with a capacity)";

// lpipsPyTorch/modules/lpips.py:32 for the SECOND image alone: feat_y = self.net(y), kept raw (line 34's normalisation is the tap's)
static int lpips_reference(const char* me, const moss_lpips_vgg_reference_args* a, Precision prec, void* stream)
{
    if (!a) return invalid_arg(me, "null argument block");
    int FH = a->frame_H, FW = a->frame_W;
    int H = a->H, W = a->W;
    if (const char* why = check_frame(H, W, a->cap_H, a->cap_W, a->rect, FH, FW)) return invalid_arg(me, why);
    if (!a->y) return invalid_arg(me, "null y");
    if (!a->shift || !a->scale) return invalid_arg(me, "null shift or scale");
    if (const char* why = null_weights(a->weights, a->biases)) return invalid_arg(me, why);
    const Geo g = geometry(H, W);
    if (!a->reference || a->reference_bytes < g.reference_bytes) return invalid_arg(me, SHORT_REFERENCE);
    if (!a->workspace || a->workspace_bytes < g.workspace_bytes) return invalid_arg(me, SHORT_WORKSPACE);
    const FwdCall f{a->y, nullptr, nullptr, a->reference, a->rect, a->cap_H, a->cap_W, a->weights, a->biases, nullptr, a->shift,
                    a->scale, nullptr, nullptr, nullptr, a->workspace};
    forward_launches(f, g, H, W, FH, FW, prec, (hipStream_t)stream);
    return launch_status(me);
}

// lpipsPyTorch/modules/lpips.py:31-37 with feat_y (line 32) read from a reference block instead of computed
static int lpips_forward_ref(const char* me, const moss_lpips_vgg_forward_ref_args* a, Precision prec, void* stream)
{
    if (!a) return invalid_arg(me, "null argument block");
    int FH = a->frame_H, FW = a->frame_W;
    int H = a->H, W = a->W;
    if (const char* why = check_frame(H, W, a->cap_H, a->cap_W, a->rect, FH, FW)) return invalid_arg(me, why);
    if (!a->x) return invalid_arg(me, "null x");
    if (!a->out) return invalid_arg(me, "null out");
    if (!a->shift || !a->scale) return invalid_arg(me, "null shift or scale");
    if (const char* why = null_weights(a->weights, a->biases)) return invalid_arg(me, why);
    for (int l = 0; l < NTAP; l++)
        if (!a->lin[l]) return invalid_arg(me, "null lin weight (5)");
    const Geo g = geometry(H, W);
    if (!a->reference || a->reference_bytes < g.reference_bytes) return invalid_arg(me, SHORT_REFERENCE);
    if (!a->workspace || a->workspace_bytes < g.workspace_bytes) return invalid_arg(me, SHORT_WORKSPACE);
    const FwdCall f{a->x, nullptr, a->reference, nullptr, a->rect, a->cap_H, a->cap_W, a->weights, a->biases, a->lin, a->shift,
                    a->scale, a->out, a->terms, a->saved, a->workspace};
    forward_launches(f, g, H, W, FH, FW, prec, (hipStream_t)stream);
    return launch_status(me);
}

extern "C" int moss_lpips_vgg_forward(const moss_lpips_vgg_args* a, void* stream)
{
    return lpips_forward("moss_lpips_vgg_forward", a, PREC_F32, stream);
}

extern "C" int moss_lpips_vgg_forward_bf16(const moss_lpips_vgg_args* a, void* stream)
{
    return lpips_forward("moss_lpips_vgg_forward_bf16", a, PREC_BF16, stream);
}

extern "C" int moss_lpips_vgg_forward_bf16x3(const moss_lpips_vgg_args* a, void* stream)
{
    return lpips_forward("moss_lpips_vgg_forward_bf16x3", a, PREC_BF16X3, stream);
}

extern "C" size_t moss_lpips_vgg_reference_bytes(int H, int W) { return size_ok(H, W) ? geometry(H, W).reference_bytes : 0; }

extern "C" int moss_lpips_vgg_reference(const moss_lpips_vgg_reference_args* a, void* stream)
{
    return lpips_reference("moss_lpips_vgg_reference", a, PREC_F32, stream);
}

extern "C" int moss_lpips_vgg_reference_bf16(const moss_lpips_vgg_reference_args* a, void* stream)
{
    return lpips_reference("moss_lpips_vgg_reference_bf16", a, PREC_BF16, stream);
}

extern "C" int moss_lpips_vgg_reference_bf16x3(const moss_lpips_vgg_reference_args* a, void* stream)
{
    return lpips_reference("moss_lpips_vgg_reference_bf16x3", a, PREC_BF16X3, stream);
}

extern "C" int moss_lpips_vgg_forward_ref(const moss_lpips_vgg_forward_ref_args* a, void* stream)
{
    return lpips_forward_ref("moss_lpips_vgg_forward_ref", a, PREC_F32, stream);
}

extern "C" int moss_lpips_vgg_forward_ref_bf16(const moss_lpips_vgg_forward_ref_args* a, void* stream)
{
    return lpips_forward_ref("moss_lpips_vgg_forward_ref_bf16", a, PREC_BF16, stream);
}

extern "C" int moss_lpips_vgg_forward_ref_bf16x3(const moss_lpips_vgg_forward_ref_args* a, void* stream)
{
    return lpips_forward_ref("moss_lpips_vgg_forward_ref_bf16x3", a, PREC_BF16X3, stream);
}

// the adjoint of LPIPS.forward (lpipsPyTorch/modules/lpips.py:31-37) w.r.t. x.  prec: weights_bwd[1..12] are that precision's packing
static int lpips_backward(const char* me, const moss_lpips_vgg_backward_args* a, Precision prec, void* stream)
{
    if (!a) return invalid_arg(me, "null argument block");
    int FH = a->frame_H, FW = a->frame_W;
    int H = a->H, W = a->W;
    if (const char* why = check_frame(H, W, a->cap_H, a->cap_W, a->rect, FH, FW)) return invalid_arg(me, why);
    if (!a->saved || !a->g_out || !a->dL_dx || !a->scale) return invalid_arg(me, "null saved (the forward's), g_out, dL_dx or scale");
    for (int i = 0; i < NCONV; i++)
        if (!a->weights_bwd[i]) return invalid_arg(me, "null backward weight (13, packed by moss_lpips_vgg_pack_weights)");
    const Geo g = geometry(H, W);
    if (!a->workspace || a->workspace_bytes < g.workspace_bytes) return invalid_arg(me, SHORT_WORKSPACE);
    auto dyn_at = [&](int level) { return Dyn{a->rect, a->cap_H, a->cap_W, level}; };     // (cap_H == 0: the kernels take the sizes below)
    hipStream_t s = (hipStream_t)stream;
    float* cur = reinterpret_cast<float*>(a->workspace);
    float* nxt = reinterpret_cast<float*>(a->workspace + g.buf_bytes);
    const char* sv = a->saved;
    auto mask_at = [&](int i) { return reinterpret_cast<const uint32_t*>(sv + g.mask_off[i]); };

    // `cur` holds d z (the gradient w.r.t. the pre-activation) of convolution i at the top of each round
    const float* from_above = nullptr;
    for (int i = NCONV - 1; i >= 1; i--) {
        const int l = CONV_LEVEL[i];
        if (i == TAP_CONV[l]) {
            hipLaunchKernelGGL(unpool_tap_kernel, dim3(grid_for((long long)g.H[l] * g.W[l] * (TAP_C[l] / 4))), dim3(WG), 0, s,
                               reinterpret_cast<const float*>(sv + g.g_off[l]), from_above,
                               from_above ? reinterpret_cast<const uint32_t*>(sv + g.win_off[l]) : nullptr, mask_at(i), nxt, g.H[l], g.W[l],
                               TAP_C[l], dyn_at(l));
            std::swap(cur, nxt);
        }
        const bool pooled_below = CONV_LEVEL[i - 1] != l;                // the input of convolution i is a pool's output
        ConvArgs c{};
        c.in = cur; c.w = a->weights_bwd[i]; c.out = nxt; c.mask_in = pooled_below ? nullptr : mask_at(i - 1);
        c.M = g.H[l] * g.W[l]; c.H = g.H[l]; c.W = g.W[l]; c.Cin = CONV_COUT[i]; c.Cout = CONV_COUT[i - 1];
        c.dyn = dyn_at(l); c.nimg = 1;
        if (pooled_below) launch_conv<MODE_BWD_PLAIN>(c, prec, s); else launch_conv<MODE_BWD_MASK>(c, prec, s);
        std::swap(cur, nxt);
        from_above = pooled_below ? cur : nullptr;
    }
    hipLaunchKernelGGL(conv_first_backward_kernel, dim3(grid_for((long long)FH * FW)), dim3(WG), 0, s, (const float*)cur, a->rect, FH, FW,
                       H, W, a->weights_bwd[0], a->scale, a->g_out, a->dL_dx, dyn_at(0));
    return launch_status(me);
}

extern "C" int moss_lpips_vgg_backward(const moss_lpips_vgg_backward_args* a, void* stream)
{
    return lpips_backward("moss_lpips_vgg_backward", a, PREC_F32, stream);
}

extern "C" int moss_lpips_vgg_backward_bf16(const moss_lpips_vgg_backward_args* a, void* stream)
{
    return lpips_backward("moss_lpips_vgg_backward_bf16", a, PREC_BF16, stream);
}

extern "C" int moss_lpips_vgg_backward_bf16x3(const moss_lpips_vgg_backward_args* a, void* stream)
{
    return lpips_backward("moss_lpips_vgg_backward_bf16x3", a, PREC_BF16X3, stream);
}

// ONE wide convolution, through launch_conv with the kernel shape the caller names: the product's own instantiations, a layer at a time
// split: the call of moss_lpips_vgg_conv3x3_bf16x3 (weights are the split packing, the bf16 field must be 0)
static int conv3x3_layer(const char* me, const moss_lpips_conv3x3_args* a, bool split, void* stream)
{
    if (!a) return invalid_arg(me, "null argument block");
    if (a->mode < MODE_FWD || a->mode > MODE_BWD_PLAIN) return invalid_arg(me, "mode must be 0 (forward), 1 (data gradient, masked) or 2 (data gradient, plain)");
    if (a->shape < SHAPE_AUTO || a->shape > SHAPE_ROWS32) return invalid_arg(me, "shape must be 0 (the launcher's choice), 1 (128 rows) or 2 (32 rows, split K)");
    if (split) {
        if (a->bf16 != 0) return invalid_arg(me, "bf16 must be 0: the split-bf16 convolution has an entry point of its own");
    } else if (a->bf16 != 0 && a->bf16 != 1) {
        return invalid_arg(me, "bf16 must be 0 or 1");
    }
    if (a->nimg < 1 || a->nimg > 2) return invalid_arg(me, "nimg must be 1 or 2");
    if (a->cin < 64 || a->cout < 64 || a->cin % 64 || a->cout % 64) return invalid_arg(me, "cin and cout must be positive multiples of 64");
    if (!a->in || !a->weights || !a->out) return invalid_arg(me, "null in, weights or out");
    if (a->mode == MODE_FWD && !a->bias) return invalid_arg(me, "the forward needs bias");
    if (a->mode == MODE_BWD_MASK && !a->mask_in) return invalid_arg(me, "the masked data gradient needs mask_in");
    int H = a->H, W = a->W, level = 0;
    if (a->cap_H || a->cap_W) {
        if (a->cap_H <= 0 || a->cap_W <= 0) return invalid_arg(me, "cap_H and cap_W must both be set (or both 0: the static call)");
        if (!a->rect) return invalid_arg(me, "a capacity needs rect: the size is read from it on the device");
        if (!size_ok(a->cap_H, a->cap_W)) return invalid_arg(me, "the capacity must be >= 16 per axis, cap_H <= 32768, cap_W <= 65536 and cap_H * cap_W <= 2^22");
        if (a->level < 0 || a->level > 4) return invalid_arg(me, "level must be 0..4");
        level = a->level;
        H = a->cap_H >> level; W = a->cap_W >> level;
    } else {
        if (H < 1 || W < 1) return invalid_arg(me, "H and W must be >= 1");
        if (!packing_ok(H, W) || (long long)H * W > (1ll << 22)) return invalid_arg(me, "H <= 32768, W <= 65536 and H * W <= 2^22");
    }
    ConvArgs c{};
    c.in = a->in; c.w = static_cast<const float*>(a->weights); c.out = a->out;
    c.bias = a->mode == MODE_FWD ? a->bias : nullptr;
    c.mask_in = a->mode == MODE_BWD_MASK ? a->mask_in : nullptr;
    c.mask_out = a->mode == MODE_FWD ? a->mask_out : nullptr;
    c.M = a->nimg * H * W; c.mask_rows = H * W; c.H = H; c.W = W; c.Cin = a->cin; c.Cout = a->cout;
    c.dyn = Dyn{a->rect, a->cap_H, a->cap_W, level}; c.nimg = a->nimg;
    hipStream_t s = (hipStream_t)stream;
    const Precision prec = split ? PREC_BF16X3 : a->bf16 ? PREC_BF16 : PREC_F32;
    if (a->mode == MODE_FWD) launch_conv<MODE_FWD>(c, prec, s, a->shape);
    else if (a->mode == MODE_BWD_MASK) launch_conv<MODE_BWD_MASK>(c, prec, s, a->shape);
    else launch_conv<MODE_BWD_PLAIN>(c, prec, s, a->shape);
    return launch_status(me);
}

extern "C" int moss_lpips_vgg_conv3x3(const moss_lpips_conv3x3_args* a, void* stream)
{
    return conv3x3_layer("moss_lpips_vgg_conv3x3", a, false, stream);
}

extern "C" int moss_lpips_vgg_conv3x3_bf16x3(const moss_lpips_conv3x3_args* a, void* stream)
{
    return conv3x3_layer("moss_lpips_vgg_conv3x3_bf16x3", a, true, stream);
}
