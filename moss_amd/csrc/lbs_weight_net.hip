// lbs_weight_net.hip -- MOSS's LBS-weight network, CrossAttention_lbs.forward (nets/mlp_delta_weight_lbs.py:31-54), and its adjoint
// (include/moss_raster.h moss_lbs_weight_net_forward / _backward).
//
// Per point x (3), with the frame's refined rotations Rs (23,3,3):
//     e (63)  = [x, sin(x 2^0), cos(x 2^0), ..., sin(x 2^9), cos(x 2^9)]           (accurate sincosf: the arguments reach +-512)
//     h0 = relu(W0 e + b0), h1 = relu(W1 h0 + b1), h2 = relu(W2 h1 + b2), h3 = relu(W3 [e ; h2] + b3)
//     q0 = Wfc h3 + bfc (24),  Q = Wq q0 + bq (24)
//     M (24,9) = a row of ONES, then Rs[j] flattened;  K = M Wk^T + bk,  V = M Wv^T + bv
//     s = Q . K / sqrt(24) (9),  a = softmax(s),  out[j] = sum_c a[c] V[j,c] (24)
// MOSS runs this as ~40 torch launches over all P Gaussians (MIOpen / hipBLASLt GEMMs, every hidden activation through HBM several
// times).  Here every product with a 128-wide side runs on the f32-input matrix cores (v_mfma_f32_32x32x2_f32: exact float32, an
// ordered fmaf chain), a 32x32 output block per wave:
//   forward, ONE launch: a workgroup of 4 waves owns 32 points.  The activations of the tile live in LDS (A operand: lane = point),
//     the weights are read from L2 as the B operand (lane = output channel; wave w owns channels 32 w ...).  A lane reads FOUR
//     consecutive k of its row at once and the four MFMAs that follow take k = k0 + 4 (lane / 32) + s from both operands: the order
//     of the contraction index is free as long as A and B agree.  bw_fc (24 outputs: one block) is split over the four waves by k and
//     summed in wave order.  Q, the scores, the softmax and the output: eight threads per point.  K and V are formed by every
//     workgroup.  Per point the kernel reads x and writes out and -- for a backward -- one row of `saved`.
//   backward, THREE launches (the activations are SAVED, not recomputed: DESIGN 4.14):
//     1. data gradients, per tile of 32 points: softmax / attention adjoint, then d(pre-activation) of bw_fc and the four layers
//        back to front (B operand = the weight rows as stored: coalesced), each written to the workspace; g_x from d e.
//     2. weight gradients: dW[n][k] = sum_p dz[p][n] in[p][k], a matrix product over the POINTS.  Both operands are read straight
//        from global memory in the layout the MFMA wants (lane = column).  A wave owns one (32 x 64) block of one tensor and one of
//        MOSS_LBS_WEIGHT_NET_SPLITS fixed ranges of points; it writes its partial block.  The biases are the column sums of dz
//        (a VALU add beside the MFMAs); d K and d V (24 x 9, sums over the points too) are two more blocks of the same machinery.
//     3. fold: the partial blocks are summed in split order into the 12 gradient tensors; one more workgroup folds d K, d V and
//        forms the gradients of key.*, value.* and Rs from them.
// Every sum has a fixed order and there is no atomic: results are bitwise reproducible.  Every output element is written.
//
// The forward, data-gradient and weight-gradient kernels are templates with two instantiations each: <false> is the f32 mode above,
// <true> the opt-in split-bf16 mode (moss_lbs_weight_net_forward_bf16x3 / _backward_bf16x3), which runs the five wide products on
// v_mfma_f32_32x32x16_bf16 with both operands split in two bf16 halves and three products per product.  What a mode contributes is its
// OPERAND POLICY (TileF32 / TileSplit below: the LDS tile, put() and the two products over it) and its loop in the weight-gradient
// kernel.  Everything else -- the embedding, the head, the attention adjoint, the ReLU masks, g_x, the layouts of `saved` and the
// workspace, the launches and the order rules -- is float32, stated once, and the same in both.
#include <type_traits>

#include "common.h"
#include "mfma_bf16.h"

namespace moss {

namespace {

constexpr int NPAR = MOSS_LBS_WEIGHT_NET_PARAMS;
constexpr int T = 32;                      // points per workgroup
constexpr int WG = 256;                    // 4 waves
constexpr int NE = 63, NH = 128, NF = 24, NC = 9, NR = 24, NFREQ = 10;
constexpr int W3_LD = NE + NH;             // 191
// parameter indices (the state_dict order of the header)
enum { P_W0, P_B0, P_W1, P_B1, P_W2, P_B2, P_W3, P_B3, P_WFC, P_BFC, P_WQ, P_BQ, P_WK, P_BK, P_WV, P_BV };
// a row of `saved` (floats): [e, one zero, h2] is contiguous, as layer 3 reads it
constexpr int SV_H0 = 0, SV_H1 = 128, SV_E = 256, SV_H2 = 320, SV_H3 = 448, SV_Q0 = 576, SV_Q = 600, SV_A = 624, SV_ROW = 640;
static_assert(SV_ROW == MOSS_LBS_WEIGHT_NET_SAVED_FLOATS, "saved row");
// a row of the backward's workspace (floats): d pre-activations of the four layers, d q0, d Q, d s / sqrt(24)
constexpr int WS_DZ0 = 0, WS_DZ1 = 128, WS_DZ2 = 256, WS_DZ3 = 384, WS_DQ0 = 512, WS_DQ = 536, WS_DS = 560, WS_ROW = 576;
// the flat gradient vector of a split: the 12 tensors of the network in order, then d K and d V (24 x 9 each)
constexpr int G_W0 = 0, G_B0 = G_W0 + NH * NE, G_W1 = G_B0 + NH, G_B1 = G_W1 + NH * NH, G_W2 = G_B1 + NH, G_B2 = G_W2 + NH * NH,
              G_W3 = G_B2 + NH, G_B3 = G_W3 + NH * W3_LD, G_WFC = G_B3 + NH, G_BFC = G_WFC + NF * NH, G_WQ = G_BFC + NF,
              G_BQ = G_WQ + NF * NF, G_NET = G_BQ + NF, G_DK = G_NET, G_DV = G_DK + NR * NC, G_ALL = G_DV + NR * NC;
static_assert(G_NET == 69488, "flat gradient layout");
constexpr int SPLITS = MOSS_LBS_WEIGHT_NET_SPLITS;

// ---- the operand policies ------------------------------------------------------------------------------------------------------------
// A wide product reads its A operand (lane = point) from an LDS tile of T rows and COLS columns, Tile<SPLIT, COLS>: put() stores a
// float32 value in the tile's format, row() is what a lane hands to gemm_wt (activation x weight^T) and gemm_w (the adjoint products),
// which are overloaded on it.  A tile occupies FLOATS floats of LDS in either format.
//   TileF32: floats; a lane reads four consecutive k, the wave takes eight per step on v_mfma_f32_32x32x2_f32.
//   TileSplit: two bf16 planes, hi = bf16(a) and lo = bf16(a - hi) (mfma_bf16.h), a value split ONCE, when it is put; a lane reads eight
//     consecutive k of each plane, the wave takes sixteen per step on v_mfma_f32_32x32x16_bf16, and a b is taken as
//     lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b), accumulated in float32.  The weights change every step, so there is no pack-once: a
//     weight is split in registers as it is read.  K = 63 pads to 64 and 191 to 192 through the same [e, 0, h2] row as in f32.
// `saved` and the workspace are float32 in both modes (the ReLU masks, the biases' column sums, query / key / value and the head read
// them), so the two size queries serve both.
template <int COLS>
struct TileF32 {
    static constexpr int LD = COLS + 4;      // row stride (floats) = 4 mod 64: the 32 lanes of a half wave read their float4 from 32 different bank groups
    static constexpr int FLOATS = T * LD;
    float* p;
    __device__ __forceinline__ explicit TileF32(float* lds) : p(lds) {}
    __device__ __forceinline__ void put(int row, int col, float v) const { p[row * LD + col] = v; }
    __device__ __forceinline__ const float* row(int r) const { return p + r * LD; }
};

struct RowSplit { const __bf16 *hi, *lo; };

template <int COLS>
struct TileSplit {
    static constexpr int LD = COLS + 8;      // row stride (bf16) of a plane: an odd multiple of 16 bytes mod 256
    static constexpr int FLOATS = T * LD;    // the pair of planes
    __bf16 *hi, *lo;
    __device__ __forceinline__ explicit TileSplit(float* lds) : hi(reinterpret_cast<__bf16*>(lds)), lo(hi + T * LD) {}
    __device__ __forceinline__ void put(int row, int col, float v) const
    {
        __bf16 h, l;
        split_bf16(v, h, l);
        hi[row * LD + col] = h;
        lo[row * LD + col] = l;
    }
    __device__ __forceinline__ RowSplit row(int r) const { return {hi + r * LD, lo + r * LD}; }
};

template <bool SPLIT, int COLS>
using Tile = typename std::conditional<SPLIT, TileSplit<COLS>, TileF32<COLS>>::type;

// A tile of NH columns also serves as plain floats once its last reader has passed a barrier: the four 32 x 32 partial blocks of
// bw_fc (forward), d e as a float tile of stride H_LD (data gradient)
constexpr int H_LD = TileF32<NH>::LD;
static_assert(TileF32<NH>::FLOATS >= 4 * 1024 && TileSplit<NH>::FLOATS >= 4 * 1024 && TileSplit<NH>::FLOATS >= T * H_LD, "aliased LDS tile");

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at a float's alignment (a weight row starts anywhere)

// acc[pt][n] += sum_{k in [kbase, kbase + K)} A[pt][k] W[n][k]: A in LDS (a_row = this lane's point), W (out, LD) row-major in
// global memory.  SKIP: A is [e (63), 0, h2 (128)] and W is W3 (LD = 191): column 63 of A has no weight.
template <int K, int LD, bool SKIP>
__device__ __forceinline__ f32x16 gemm_wt(const float* __restrict__ W, int n, bool n_ok, const float* a_row, int half, f32x16 acc,
                                          int kbase = 0)
{
    const float* w = W + (size_t)(n_ok ? n : 0) * LD;
#pragma unroll 2
    for (int k0 = kbase; k0 < kbase + K; k0 += 8) {
        const int kk = k0 + 4 * half;
        const float4 av = *reinterpret_cast<const float4*>(a_row + kk);
        float bv[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int k = kk + s;
            const bool ok = n_ok && (SKIP ? k != NE : k < LD);
            const int kw = SKIP ? (k < NE ? k : k - 1) : k;
            bv[s] = ok ? w[kw] : 0.0f;
        }
        mfma4(acc, av, bv);
    }
    return acc;
}

template <int K, int LD, bool SKIP>
__device__ __forceinline__ f32x16 gemm_wt(const float* __restrict__ W, int n, bool n_ok, const RowSplit a_row, int half, f32x16 acc,
                                          int kbase = 0)
{
    const float* w = W + (size_t)(n_ok ? n : 0) * LD;
#pragma unroll 2
    for (int k0 = kbase; k0 < kbase + K; k0 += 16) {
        const int kk = k0 + 8 * half;
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_row.hi + kk), al = *reinterpret_cast<const bf16x8*>(a_row.lo + kk);
        // this lane's eight weights: W[n][kk ...] (SKIP: the row without its column 63), as two 16-byte reads where all eight exist
        const int first = SKIP && kk > NE ? kk - 1 : kk, valid = SKIP ? (kk + 8 == NE + 1 ? 7 : 8) : min(8, LD - kk);
        float bv[8];
        if (n_ok && valid == 8) {
            const f32x4u lo4 = *reinterpret_cast<const f32x4u*>(w + first), hi4 = *reinterpret_cast<const f32x4u*>(w + first + 4);
#pragma unroll
            for (int s = 0; s < 4; s++) { bv[s] = lo4[s]; bv[4 + s] = hi4[s]; }
        } else {
#pragma unroll
            for (int s = 0; s < 8; s++) bv[s] = n_ok && s < valid ? w[first + s] : 0.0f;
        }
        bf16x8 bh, bl;
        split_bf16x8(bv, bh, bl);
        mfma16x3(acc, ah, al, bh, bl);
    }
    return acc;
}

// acc[pt][col] = sum_{k < K} A[pt][k] W[k][col] (rows k >= kvalid and a column that is not ok count as zero): the adjoint products
template <int K>
__device__ __forceinline__ f32x16 gemm_w(const float* __restrict__ W, int ld, int kvalid, int col, bool col_ok, const float* a_row, int half)
{
    f32x16 acc = splat(0.0f);
    const float* w = W + (col_ok ? col : 0);
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 8) {
        const int kk = k0 + 4 * half;
        const float4 av = *reinterpret_cast<const float4*>(a_row + kk);
        float bv[4];
#pragma unroll
        for (int s = 0; s < 4; s++) bv[s] = (col_ok && kk + s < kvalid) ? w[(size_t)(kk + s) * ld] : 0.0f;
        mfma4(acc, av, bv);
    }
    return acc;
}

template <int K>
__device__ __forceinline__ f32x16 gemm_w(const float* __restrict__ W, int ld, int kvalid, int col, bool col_ok, const RowSplit a_row, int half)
{
    f32x16 acc = splat(0.0f);
    const float* w = W + (col_ok ? col : 0);
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kk = k0 + 8 * half;
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_row.hi + kk), al = *reinterpret_cast<const bf16x8*>(a_row.lo + kk);
        float bv[8];
#pragma unroll
        for (int s = 0; s < 8; s++) bv[s] = (col_ok && kk + s < kvalid) ? w[(size_t)(kk + s) * ld] : 0.0f;
        bf16x8 bh, bl;
        split_bf16x8(bv, bh, bl);
        mfma16x3(acc, ah, al, bh, bl);
    }
    return acc;
}

// ---- the phases both modes share (float32) -------------------------------------------------------------------------------------------

// relu(acc) -> the tile [row][col] and, with `saved`, the rows of the points that exist
template <class TileT>
__device__ __forceinline__ void store_act(const f32x16& acc, const TileT& tile, int col, int half, float* saved, int sv_col, int p0, int P)
{
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = acc_row(r, half);
        const float v = fmaxf(acc[r], 0.0f);
        tile.put(row, col, v);
        if (saved && p0 + row < P) saved[(size_t)(p0 + row) * SV_ROW + sv_col] = v;
    }
}

// K = M Wk^T + bk, V = M Wv^T + bv (24 x 9) and a copy of Wq, in LDS
struct alignas(16) HeadConstants { float K[NR * NC], V[NR * NC], Wq[NF * NF]; };

// (no barrier inside)
__device__ __forceinline__ void head_constants(const float* __restrict__ Rs, const float* const* par, HeadConstants& hc, int tid)
{
    if (tid < NR * NC) {
        const int r = tid / NC, c = tid % NC;
        float k = par[P_BK][c], v = par[P_BV][c];
#pragma unroll
        for (int i = 0; i < NC; i++) {
            const float m = r == 0 ? 1.0f : Rs[(r - 1) * NC + i];
            k = __fmaf_rn(m, par[P_WK][c * NC + i], k);
            v = __fmaf_rn(m, par[P_WV][c * NC + i], v);
        }
        hc.K[tid] = k;
        hc.V[tid] = v;
    }
    for (int i = tid; i < NF * NF; i += WG) hc.Wq[i] = par[P_WQ][i];
}

// [e (63), 0] of the tile's points -> columns 0 .. 63 of the tile and, with `saved`, of the rows of the points that exist (no barrier inside)
template <class TileT>
__device__ __forceinline__ void embed(const float* __restrict__ x, const TileT& eh, float* saved, int p0, int P, int tid)
{
    for (int i = tid; i < T * 3 * NFREQ; i += WG) {
        const int pt = i / (3 * NFREQ), r = i % (3 * NFREQ), f = r / 3, d = r % 3;
        const float xv = p0 + pt < P ? x[(size_t)(p0 + pt) * 3 + d] : 0.0f;
        float sn, cs;
        sincosf(xv * (float)(1 << f), &sn, &cs);
        float* sv = saved && p0 + pt < P ? saved + (size_t)(p0 + pt) * SV_ROW + SV_E : nullptr;
        auto put = [&](int k, float v) {
            eh.put(pt, k, v);
            if (sv) sv[k] = v;
        };
        put(3 + 6 * f + d, sn);
        put(6 + 6 * f + d, cs);
        if (f == 0) put(d, xv);
        if (r == 0) put(NE, 0.0f);
    }
}

// the forward's head, eight threads per point: q0 from bw_fc's four partial blocks (`part`: 4 x 32 x 32 floats, summed in wave
// order), Q, the scores, the softmax, out; with `saved`, q0, Q, a and the row's padding.  The caller's barrier precedes it.
struct alignas(16) ForwardHeadLds { float q0[T][NF], Q[T][NF], s[T][12]; };

__device__ __forceinline__ void forward_head(const moss_lbs_weight_net_args& a, const float* part, const HeadConstants& hc, ForwardHeadLds& s,
                                             int p0, int tid)
{
    const float* const* par = a.params;
    const int pt = tid >> 3, sub = tid & 7;
    const bool live = p0 + pt < a.P;
    float* sv = a.saved && live ? a.saved + (size_t)(p0 + pt) * SV_ROW : nullptr;
#pragma unroll
    for (int k = sub; k < NF; k += 8) {
        const float* q = part + pt * 32 + k;
        const float v = (((q[0] + q[1024]) + q[2048]) + q[3072]) + par[P_BFC][k];
        s.q0[pt][k] = v;
        if (sv) sv[SV_Q0 + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = sub; i < NF; i += 8) {
        float v = par[P_BQ][i];
#pragma unroll
        for (int k = 0; k < NF; k++) v = __fmaf_rn(hc.Wq[i * NF + k], s.q0[pt][k], v);
        s.Q[pt][i] = v;
        if (sv) sv[SV_Q + i] = v;
    }
    __syncthreads();
    for (int c = sub; c < NC; c += 8) {
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < NF; i++) v = __fmaf_rn(s.Q[pt][i], hc.K[i * NC + c], v);
        s.s[pt][c] = v / sqrtf((float)NF);
    }
    __syncthreads();
    float att[NC], m = s.s[pt][0], sum = 0.0f;
#pragma unroll
    for (int c = 1; c < NC; c++) m = fmaxf(m, s.s[pt][c]);
#pragma unroll
    for (int c = 0; c < NC; c++) { att[c] = expf(s.s[pt][c] - m); sum += att[c]; }
#pragma unroll
    for (int c = 0; c < NC; c++) att[c] /= sum;
    if (sv) {
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < NC; c++) sv[SV_A + c] = att[c];
        } else if (sub == 1) {
#pragma unroll
            for (int c = NC; c < SV_ROW - SV_A; c++) sv[SV_A + c] = 0.0f;      // (the row's padding: defined, never read)
        }
    }
    if (live) {
#pragma unroll
        for (int o = sub; o < NR; o += 8) {
            float v = 0.0f;
#pragma unroll
            for (int c = 0; c < NC; c++) v = __fmaf_rn(att[c], hc.V[o * NC + c], v);
            a.out[(size_t)(p0 + pt) * NR + o] = v;
        }
    }
}

// the backward's first phase, eight threads per point: d a, d s / sqrt(24), d Q and d q0 from g_out and the saved softmax; d s, d Q and
// d q0 go to the workspace (with the row's padding), d q0 also into the tile `dq0`, whose padding columns are zeroed.  Ends in a barrier.
struct alignas(16) AdjointLds { float g[T][NR], att[T][12], da[T][12], ds[T][12], dQ[T][NF]; };

template <class TileT>
__device__ __forceinline__ void attention_adjoint(const moss_lbs_weight_net_backward_args& a, float* __restrict__ ws, const HeadConstants& hc,
                                                  AdjointLds& s, const TileT& dq0, int p0, int tid)
{
    constexpr int PAD = TileT::LD - NF;
    const int P = a.P;
    for (int i = tid; i < T * NR; i += WG) {
        const int pt = i / NR;
        s.g[pt][i % NR] = p0 + pt < P ? a.g_out[(size_t)p0 * NR + i] : 0.0f;
    }
    for (int i = tid; i < T * NC; i += WG) {
        const int pt = i / NC, c = i % NC;
        s.att[pt][c] = p0 + pt < P ? a.saved[(size_t)(p0 + pt) * SV_ROW + SV_A + c] : 0.0f;
    }
    for (int i = tid; i < T * PAD; i += WG) dq0.put(i / PAD, NF + i % PAD, 0.0f);
    __syncthreads();

    const int pt = tid >> 3, sub = tid & 7;
    const bool live = p0 + pt < P;
    float* wrow = live ? ws + (size_t)(p0 + pt) * WS_ROW : nullptr;
    for (int c = sub; c < NC; c += 8) {
        float v = 0.0f;
#pragma unroll
        for (int o = 0; o < NR; o++) v = __fmaf_rn(s.g[pt][o], hc.V[o * NC + c], v);
        s.da[pt][c] = v;
    }
    __syncthreads();
    {
        float dot = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++) dot = __fmaf_rn(s.att[pt][c], s.da[pt][c], dot);
        for (int c = sub; c < NC; c += 8) {
            const float v = s.att[pt][c] * (s.da[pt][c] - dot) / sqrtf((float)NF);
            s.ds[pt][c] = v;
            if (wrow) wrow[WS_DS + c] = v;
        }
        if (wrow && sub == 7)
            for (int c = NC; c < WS_ROW - WS_DS; c++) wrow[WS_DS + c] = 0.0f;   // (the row's padding: defined, never read)
    }
    __syncthreads();
#pragma unroll
    for (int i = sub; i < NF; i += 8) {
        float v = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++) v = __fmaf_rn(s.ds[pt][c], hc.K[i * NC + c], v);
        s.dQ[pt][i] = v;
        if (wrow) wrow[WS_DQ + i] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = sub; k < NF; k += 8) {
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < NF; i++) v = __fmaf_rn(hc.Wq[i * NF + k], s.dQ[pt][i], v);
        dq0.put(pt, k, v);
        if (wrow) wrow[WS_DQ0 + k] = v;
    }
    __syncthreads();
}

// g_x from d e: `de` is a float tile of stride H_LD whose columns 0 .. 62 and 64 .. 126 hold the two halves of d e (W3's and W0's)
__device__ __forceinline__ void gx_tail(const moss_lbs_weight_net_backward_args& a, const float* de, int p0, int tid)
{
    if (tid < T * 3) {
        const int q = tid / 3, d = tid % 3;
        if (p0 + q < a.P) {
            const float* z = de + q * H_LD;
            const float* e = a.saved + (size_t)(p0 + q) * SV_ROW + SV_E;
            float v = z[d] + z[64 + d];
#pragma unroll
            for (int f = 0; f < NFREQ; f++) {
                const int is = 3 + 6 * f + d, ic = is + 3;
                const float dsn = z[is] + z[64 + is], dcs = z[ic] + z[64 + ic];
                v += (float)(1 << f) * (e[ic] * dsn - e[is] * dcs);
            }
            a.g_x[(size_t)(p0 + q) * 3 + d] = v;
        }
    }
}

// ---- the kernels: <false> the f32 mode, <true> the split-bf16 mode -------------------------------------------------------------------------

template <bool SPLIT>
__global__ void __launch_bounds__(WG)
lbs_weight_net_forward_kernel(const moss_lbs_weight_net_args a)
{
    typedef Tile<SPLIT, 64 + NH> TileEH;
    typedef Tile<SPLIT, NH> TileH;
    __shared__ __attribute__((aligned(16))) float s_eh[TileEH::FLOATS], s_a[TileH::FLOATS], s_b[TileH::FLOATS];
    __shared__ HeadConstants s_hc;
    __shared__ ForwardHeadLds s_head;
    const TileEH t_eh(s_eh);                                            // [e (63), 0, h2 (128)]
    const TileH t_a(s_a), t_b(s_b);                                     // (s_b: then bw_fc's four partial blocks, as floats)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int p0 = blockIdx.x * T, P = a.P;
    const float* const* par = a.params;
    float* saved = a.saved;

    head_constants(a.Rs, par, s_hc, tid);
    embed(a.x, t_eh, saved, p0, P, tid);
    __syncthreads();

    const int n = 32 * wave + j;                                        // this lane's output channel in the 128-wide layers
    f32x16 acc = gemm_wt<64, NE, false>(par[P_W0], n, true, t_eh.row(j), half, splat(par[P_B0][n]));
    store_act(acc, t_a, n, half, saved, SV_H0 + n, p0, P);
    __syncthreads();
    acc = gemm_wt<NH, NH, false>(par[P_W1], n, true, t_a.row(j), half, splat(par[P_B1][n]));
    store_act(acc, t_b, n, half, saved, SV_H1 + n, p0, P);
    __syncthreads();
    acc = gemm_wt<NH, NH, false>(par[P_W2], n, true, t_b.row(j), half, splat(par[P_B2][n]));
    store_act(acc, t_eh, 64 + n, half, saved, SV_H2 + n, p0, P);
    __syncthreads();                                                    // (h1 in s_b was last read before this barrier)
    acc = gemm_wt<64 + NH, W3_LD, true>(par[P_W3], n, true, t_eh.row(j), half, splat(par[P_B3][n]));
    store_act(acc, t_a, n, half, saved, SV_H3 + n, p0, P);
    __syncthreads();
    // bw_fc: one 32 x 32 block (24 channels), the k range split over the waves; the four partial blocks go to s_b
    acc = gemm_wt<NH / 4, NH, false>(par[P_WFC], j, j < NF, t_a.row(j), half, splat(0.0f), (NH / 4) * wave);
#pragma unroll
    for (int r = 0; r < 16; r++) s_b[wave * 1024 + acc_row(r, half) * 32 + j] = acc[r];
    __syncthreads();
    forward_head(a, s_b, s_hc, s_head, p0, tid);
}

// backward 1: the data gradients of a tile of points
template <bool SPLIT>
__global__ void __launch_bounds__(WG)
lbs_weight_net_backward_data_kernel(const moss_lbs_weight_net_backward_args a, float* __restrict__ ws)
{
    typedef Tile<SPLIT, NH> TileH;
    typedef Tile<SPLIT, 32> TileQ;
    __shared__ __attribute__((aligned(16))) float s_x[TileH::FLOATS], s_y[TileH::FLOATS], s_z[TileH::FLOATS], s_dq0[TileQ::FLOATS];
    __shared__ HeadConstants s_hc;
    __shared__ AdjointLds s_adj;
    const TileH t_x(s_x), t_y(s_y), t_z(s_z);                           // (s_z: d z1; then d e as a float tile)
    const TileQ t_dq0(s_dq0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, half = lane >> 5;
    const int p0 = blockIdx.x * T, P = a.P;
    const float* const* par = a.params;
    const float* saved = a.saved;

    head_constants(a.Rs, par, s_hc, tid);
    attention_adjoint(a, ws, s_hc, s_adj, t_dq0, p0, tid);

    const int n = 32 * wave + j;
    // d z = (h > 0) * acc -> the tile and the workspace
    auto store_dz = [&](const f32x16& acc, const TileH& tile, int sv_col, int ws_col) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = acc_row(r, half);
            const bool ok = p0 + row < P;
            const float h = ok ? saved[(size_t)(p0 + row) * SV_ROW + sv_col + n] : 0.0f;
            const float v = h > 0.0f ? acc[r] : 0.0f;
            tile.put(row, n, v);
            if (ok) ws[(size_t)(p0 + row) * WS_ROW + ws_col + n] = v;
        }
    };
    f32x16 acc = gemm_w<32>(par[P_WFC], NH, NF, n, true, t_dq0.row(j), half);
    store_dz(acc, t_x, SV_H3, WS_DZ3);
    __syncthreads();
    acc = gemm_w<NH>(par[P_W3], W3_LD, NH, NE + n, true, t_x.row(j), half);
    store_dz(acc, t_y, SV_H2, WS_DZ2);
    __syncthreads();
    acc = gemm_w<NH>(par[P_W2], NH, NH, n, true, t_y.row(j), half);
    store_dz(acc, t_z, SV_H1, WS_DZ1);
    __syncthreads();
    acc = gemm_w<NH>(par[P_W1], NH, NH, n, true, t_z.row(j), half);
    store_dz(acc, t_y, SV_H0, WS_DZ0);                                  // (d z2 in s_y was last read before the barrier above)
    __syncthreads();
    // d e = d z3 . W3[:, :63] + d z0 . W0: two blocks of 32 columns each, one product per wave, the two halves into s_z as floats
    // (d z1 in it was last read before the barrier above)
    {
        const int col = 32 * (wave & 1) + j;
        acc = (wave >> 1) == 0 ? gemm_w<NH>(par[P_W3], W3_LD, NH, col, col < NE, t_x.row(j), half)
                               : gemm_w<NH>(par[P_W0], NE, NH, col, col < NE, t_y.row(j), half);
#pragma unroll
        for (int r = 0; r < 16; r++) s_z[acc_row(r, half) * H_LD + 64 * (wave >> 1) + col] = acc[r];
    }
    __syncthreads();
    gx_tail(a, s_z, p0, tid);
}

// backward 2: one (32 x 64) block of one weight gradient over one range of points, per wave.  In the split-bf16 mode the first
// `items.wide` items, the five wide products, take STEPS x sixteen points per iteration: a lane reads its column at eight consecutive
// points per operand and step and splits them; the bias is the float32 column sum.  Its other items (query.weight / bias, d K, d V)
// stay float32: the f32 mode's loop, in the same launch, so that their waves run beside the wide ones.
struct WgItem { int a_src, a_off, a_ld, a_n, b_src, b_off, b_ld, b_n, out_off, out_ld, bias_off; };
constexpr int MAX_ITEMS = 40;
struct WgItems { int count, wide; WgItem it[MAX_ITEMS]; };

template <bool SPLIT>
__global__ void __launch_bounds__(WG)
lbs_weight_net_backward_weights_kernel(int P, int chunk, const float* __restrict__ saved, const float* __restrict__ ws,
                                       const float* __restrict__ g_out, float* __restrict__ partial, const WgItems items)
{
    constexpr int STEPS = 2;
    const int lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
    const int id = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (id >= items.count * SPLITS) return;
    const int split = id / items.count, item = id % items.count;
    const WgItem it = items.it[item];
    const float* src[3] = {saved, ws, g_out};
    const float* A = src[it.a_src] + it.a_off + j;
    const float* B = src[it.b_src] + it.b_off + j;
    const bool a_ok = j < it.a_n, b0_ok = j < it.b_n, b1_ok = j + 32 < it.b_n;
    const int pbeg = min(P, split * chunk), pend = min(P, pbeg + chunk);
    f32x16 acc0 = splat(0.0f), acc1 = splat(0.0f);
    float bsum = 0.0f;
    const bool wide = it.b_n > 32;                                      // (wave-uniform, as is the choice of the loop)
    if (SPLIT && item < items.wide) {
        for (int q = pbeg; q < pend; q += 16 * STEPS) {                 // the loads of all steps first
            float av[STEPS][8], b0[STEPS][8], b1[STEPS][8];
#pragma unroll
            for (int t = 0; t < STEPS; t++)
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int p = q + 16 * t + 8 * half + u;
                    const bool ok = p < pend;
                    av[t][u] = ok && a_ok ? A[(size_t)p * it.a_ld] : 0.0f;
                    b0[t][u] = ok && b0_ok ? B[(size_t)p * it.b_ld] : 0.0f;
                    b1[t][u] = ok && b1_ok ? B[(size_t)p * it.b_ld + 32] : 0.0f;
                }
#pragma unroll
            for (int t = 0; t < STEPS; t++) {
                bf16x8 ah, al, bh, bl;
                split_bf16x8(av[t], ah, al);
                split_bf16x8(b0[t], bh, bl);
                mfma16x3(acc0, ah, al, bh, bl);
                if (wide) {
                    split_bf16x8(b1[t], bh, bl);
                    mfma16x3(acc1, ah, al, bh, bl);
                }
#pragma unroll
                for (int u = 0; u < 8; u++) bsum += av[t][u];
            }
        }
    } else {
        for (int q = pbeg; q < pend; q += 8) {                          // four MFMA steps of two points; the loads first
            float av[4], b0[4], b1[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int p = q + 2 * u + half;
                const bool ok = p < pend;
                av[u] = ok && a_ok ? A[(size_t)p * it.a_ld] : 0.0f;
                b0[u] = ok && b0_ok ? B[(size_t)p * it.b_ld] : 0.0f;
                b1[u] = ok && b1_ok ? B[(size_t)p * it.b_ld + 32] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], b0[u], acc0, 0, 0, 0);
                if (!SPLIT && wide) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], b1[u], acc1, 0, 0, 0);   // (the split mode's float32 items are narrow)
                bsum += av[u];
            }
        }
    }
    float* out = partial + (size_t)split * G_ALL;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = acc_row(r, half);
        if (row < it.a_n) {
            if (b0_ok) out[it.out_off + row * it.out_ld + j] = acc0[r];
            if (b1_ok) out[it.out_off + row * it.out_ld + 32 + j] = acc1[r];
        }
    }
    bsum += __shfl_xor(bsum, 32);
    if (it.bias_off >= 0 && half == 0 && a_ok) out[it.bias_off + j] = bsum;
}

struct GradPtrs { float* g[NPAR]; };

// backward 3: the partial sums in split order; the last workgroup: d K, d V -> the gradients of key.*, value.* and Rs
__global__ void __launch_bounds__(WG)
lbs_weight_net_backward_fold_kernel(const float* __restrict__ partial, const float* __restrict__ Rs, const float* __restrict__ Wk,
                                    const float* __restrict__ Wv, const GradPtrs grads, float* __restrict__ g_Rs)
{
    const int tid = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int idx = blockIdx.x * WG + tid;
        if (idx >= G_NET) return;
        float v = 0.0f;
        for (int s = 0; s < SPLITS; s++) v += partial[(size_t)s * G_ALL + idx];
        constexpr int first[13] = {G_W0, G_B0, G_W1, G_B1, G_W2, G_B2, G_W3, G_B3, G_WFC, G_BFC, G_WQ, G_BQ, G_NET};
        int t = 0;
#pragma unroll
        for (int i = 1; i < 12; i++) t += idx >= first[i];
        int base = 0;
#pragma unroll
        for (int i = 1; i < 12; i++) base = idx >= first[i] ? first[i] : base;
        grads.g[t][idx - base] = v;
        return;
    }
    __shared__ float s_dK[NR * NC], s_dV[NR * NC];
    for (int i = tid; i < 2 * NR * NC; i += WG) {
        float v = 0.0f;
        for (int s = 0; s < SPLITS; s++) v += partial[(size_t)s * G_ALL + G_DK + i];
        (i < NR * NC ? s_dK[i] : s_dV[i - NR * NC]) = v;
    }
    __syncthreads();
    if (tid < NR * NC) {
        // d M = d K Wk + d V Wv; rows 1..23 are d Rs
        const int r = tid / NC, c = tid % NC;
        if (r > 0) {
            float v = 0.0f;
#pragma unroll
            for (int o = 0; o < NC; o++) v = __fmaf_rn(s_dK[r * NC + o], Wk[o * NC + c], v);
#pragma unroll
            for (int o = 0; o < NC; o++) v = __fmaf_rn(s_dV[r * NC + o], Wv[o * NC + c], v);
            g_Rs[(r - 1) * NC + c] = v;
        }
    }
    if (tid < NC * NC) {
        // d Wk[o][c] = sum_r d K[r][o] M[r][c]
        const int o = tid / NC, c = tid % NC;
        float k = 0.0f, v = 0.0f;
        for (int r = 0; r < NR; r++) {
            const float m = r == 0 ? 1.0f : Rs[(r - 1) * NC + c];
            k = __fmaf_rn(s_dK[r * NC + o], m, k);
            v = __fmaf_rn(s_dV[r * NC + o], m, v);
        }
        grads.g[P_WK][tid] = k;
        grads.g[P_WV][tid] = v;
    } else if (tid >= 128 && tid < 128 + NC) {
        const int o = tid - 128;
        float k = 0.0f, v = 0.0f;
        for (int r = 0; r < NR; r++) { k += s_dK[r * NC + o]; v += s_dV[r * NC + o]; }
        grads.g[P_BK][o] = k;
        grads.g[P_BV][o] = v;
    }
}

void add_items(WgItems& w, int a_src, int a_off, int a_cols, int b_src, int b_off, int b_cols, int out_base, int out_ld, int bias_base)
{
    const int ld[3] = {SV_ROW, WS_ROW, NR};
    for (int n0 = 0; n0 < a_cols; n0 += 32)
        for (int k0 = 0; k0 < b_cols; k0 += 64) {
            WgItem& it = w.it[w.count++];
            it.a_src = a_src; it.a_off = a_off + n0; it.a_ld = ld[a_src]; it.a_n = std::min(32, a_cols - n0);
            it.b_src = b_src; it.b_off = b_off + k0; it.b_ld = ld[b_src]; it.b_n = std::min(64, b_cols - k0);
            it.out_off = out_base + n0 * out_ld + k0; it.out_ld = out_ld;
            it.bias_off = (k0 == 0 && bias_base >= 0) ? bias_base + n0 : -1;
        }
}

// the item table; the first `wide` items are the five wide products (what the split-bf16 mode runs on the bf16-input matrix cores)
const WgItems& weight_items()
{
    static const WgItems table = [] {
        WgItems w{};
        enum { SAVED, WS, GOUT };
        add_items(w, WS, WS_DZ0, NH, SAVED, SV_E, NE, G_W0, NE, G_B0);
        add_items(w, WS, WS_DZ1, NH, SAVED, SV_H0, NH, G_W1, NH, G_B1);
        add_items(w, WS, WS_DZ2, NH, SAVED, SV_H1, NH, G_W2, NH, G_B2);
        add_items(w, WS, WS_DZ3, NH, SAVED, SV_E, NE, G_W3, W3_LD, G_B3);
        add_items(w, WS, WS_DZ3, NH, SAVED, SV_H2, NH, G_W3 + NE, W3_LD, -1);
        add_items(w, WS, WS_DQ0, NF, SAVED, SV_H3, NH, G_WFC, NH, G_BFC);
        w.wide = w.count;
        add_items(w, WS, WS_DQ, NF, SAVED, SV_Q0, NF, G_WQ, NF, G_BQ);
        add_items(w, SAVED, SV_Q, NF, WS, WS_DS, NC, G_DK, NC, -1);       // d K[i][c] = sum_p Q[i] d s[c] / sqrt(24)
        add_items(w, GOUT, 0, NR, SAVED, SV_A, NC, G_DV, NC, -1);         // d V[j][c] = sum_p g[j] a[c]
        return w;
    }();
    return table;
}

size_t ws_rows_bytes(int P) { return align_up((size_t)P * WS_ROW * sizeof(float)); }

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_lbs_weight_net_workspace_bytes(int P)
{
    return P <= 0 ? 0 : ws_rows_bytes(P) + (size_t)SPLITS * G_ALL * sizeof(float);
}

extern "C" size_t moss_lbs_weight_net_saved_bytes(int P) { return P <= 0 ? 0 : (size_t)P * SV_ROW * sizeof(float); }

// CrossAttention_lbs.forward, nets/mlp_delta_weight_lbs.py:31-54; `fn` names the entry point in a refusal
static int forward_impl(const char* fn, const moss_lbs_weight_net_args* a, void* stream, bool bf16x3)
{
    if (!a) return invalid_arg(fn, "null argument block");
    if (a->P < 0) return invalid_arg(fn, "P must be >= 0");
    if (a->P == 0) return 0;
    if (!a->x || !a->Rs || !a->out) return invalid_arg(fn, "null x, Rs or out");
    for (int i = 0; i < NPAR; i++)
        if (!a->params[i]) return invalid_arg(fn, "null parameter tensor (all 16 are read)");
    static_assert(MAX_ITEMS >= 37, "item table");
    hipLaunchKernelGGL(bf16x3 ? lbs_weight_net_forward_kernel<true> : lbs_weight_net_forward_kernel<false>, dim3((a->P + T - 1) / T),
                       dim3(WG), 0, (hipStream_t)stream, *a);
    return launch_status(fn);
}

// the adjoint of CrossAttention_lbs.forward, nets/mlp_delta_weight_lbs.py:31-54
static int backward_impl(const char* fn, const moss_lbs_weight_net_backward_args* a, void* stream, bool bf16x3)
{
    if (!a) return invalid_arg(fn, "null argument block");
    if (a->P < 0) return invalid_arg(fn, "P must be >= 0");
    if (a->P == 0) return 0;
    if (!a->Rs || !a->saved || !a->g_out) return invalid_arg(fn, "null Rs, saved (the forward's) or g_out");
    if (!a->g_x || !a->g_Rs) return invalid_arg(fn, "null g_x or g_Rs (both are written)");
    for (int i = 0; i < NPAR; i++)
        if (!a->params[i] || !a->grads[i]) return invalid_arg(fn, "null parameter or gradient tensor (all 16 are written)");
    if (!a->workspace || a->workspace_bytes < moss_lbs_weight_net_workspace_bytes(a->P))
        return invalid_arg(fn, "the workspace is null or smaller than moss_lbs_weight_net_workspace_bytes(P)");
    const int P = a->P;
    hipStream_t s = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(a->workspace);
    float* partial = reinterpret_cast<float*>(a->workspace + ws_rows_bytes(P));
    GradPtrs gp;
    for (int i = 0; i < NPAR; i++) gp.g[i] = a->grads[i];
    const WgItems& items = weight_items();
    const dim3 grid((items.count * SPLITS + WG / 64 - 1) / (WG / 64));
    const int step = bf16x3 ? 16 : 2;                                 // the points an MFMA step takes
    const int chunk = ((P + SPLITS - 1) / SPLITS + step - 1) & ~(step - 1);   // points per split, a multiple of `step`
    hipLaunchKernelGGL(bf16x3 ? lbs_weight_net_backward_data_kernel<true> : lbs_weight_net_backward_data_kernel<false>,
                       dim3((P + T - 1) / T), dim3(WG), 0, s, *a, ws);
    hipLaunchKernelGGL(bf16x3 ? lbs_weight_net_backward_weights_kernel<true> : lbs_weight_net_backward_weights_kernel<false>, grid,
                       dim3(WG), 0, s, P, chunk, a->saved, (const float*)ws, a->g_out, partial, items);
    hipLaunchKernelGGL(lbs_weight_net_backward_fold_kernel, dim3((G_NET + WG - 1) / WG + 1), dim3(WG), 0, s, (const float*)partial,
                       a->Rs, a->params[P_WK], a->params[P_WV], gp, a->g_Rs);
    return launch_status(fn);
}

extern "C" int moss_lbs_weight_net_forward(const moss_lbs_weight_net_args* a, void* stream)
{
    return forward_impl("moss_lbs_weight_net_forward", a, stream, false);
}

extern "C" int moss_lbs_weight_net_backward(const moss_lbs_weight_net_backward_args* a, void* stream)
{
    return backward_impl("moss_lbs_weight_net_backward", a, stream, false);
}

// the same pair in the split-bf16 (three-product) mode; `saved` and the workspace have the f32 pair's sizes
extern "C" int moss_lbs_weight_net_forward_bf16x3(const moss_lbs_weight_net_args* a, void* stream)
{
    return forward_impl("moss_lbs_weight_net_forward_bf16x3", a, stream, true);
}

extern "C" int moss_lbs_weight_net_backward_bf16x3(const moss_lbs_weight_net_backward_args* a, void* stream)
{
    return backward_impl("moss_lbs_weight_net_backward_bf16x3", a, stream, true);
}
