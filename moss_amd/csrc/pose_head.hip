// pose_head.hip -- MOSS's pose-refinement head and its matrix-Fisher loss term (include/moss_raster.h moss_pose_head_forward /
// _backward, moss_matrix_fisher_nll).
//
// MOSS runs Autoregression.forward (nets/mlp_delta_body_pose.py:56-82: an MLP 69 -> 128 -> 128 -> 69, a Python loop over 23 joint
// layers, Rodrigues, torch.svd) and matrix_fisher_nll (utils/loss_utils.py:283-317: a determinant on the CPU, a 512-point quadrature,
// three more backward) as several hundred tiny launches and two host synchronisations per iteration, for 23 matrices and 36k
// weights.  The problem is latency-bound, so each direction is ONE launch of ONE 256-thread workgroup; the stages hand over through
// LDS and __syncthreads():
//   forward:  GEMV x3 (8 lanes per output row, a fixed butterfly) -> the joint layers (one thread per output, walking the parent
//             table) -> Rodrigues + SVD (one thread per joint, pose_math.h) -> the quadrature (one wave per joint: 8 points per lane,
//             then a butterfly) -> nll
//   backward: the three derivative quadratures (one wave per joint) -> dL/dRs and the Rodrigues adjoint (one thread per joint) ->
//             the joint layers (weight gradients per output; the gradient of h GATHERED per element over the joints in order: a
//             joint layer reads h of its joint and of its ancestors, and no two threads add into one address) -> the MLP: W^T g per
//             column in two halves, the outer products g (x) input written straight to the gradient tensors
// Every sum has a fixed order and there is no atomic: results are bitwise reproducible.  moss_matrix_fisher_nll runs the same SVD
// and quadrature on n general matrices, 16 per workgroup (one thread per SVD, one wave per quadrature).
#include "common.h"
#include "wave.h"
#include "pose_math.h"

namespace moss {

namespace {

using namespace pose;

constexpr int NJ = MOSS_POSE_JOINTS;       // 23
constexpr int NP = MOSS_POSE_PARAMS;       // 52
constexpr int D_IN = 3 * NJ;               // 69
constexpr int D_H = 128;
constexpr int WG = 256;
// layout of `saved` (floats)
constexpr int SV_H1 = 0, SV_H2 = 128, SV_JF = 256, SV_R = 328, SV_U = 400, SV_V = 608, SV_DET = 816, SV_CBAR = 840, SV_END = 864;
static_assert(SV_END <= MOSS_POSE_HEAD_SAVED_FLOATS, "saved block");
constexpr int NLL_PER_WG = 16;             // moss_matrix_fisher_nll: matrices per workgroup

// one wave: 0.5 * trapezoid of the integrand (times u with `with_u`); every lane returns the same bits
__device__ __forceinline__ float wave_integral(float si, float sj, float sk, bool with_u, int lane)
{
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < QUAD_POINTS / 64; i++) {
        const int p = lane + 64 * i;
        const float u = quad_u(p);
        float y = mf_integrand(si, sj, sk, u);
        if (with_u) y *= u;
        acc += quad_w(p) * y;
    }
    return quad_scale(wave_sum(acc));
}

// out[r] = act(b[r] + sum_k W[r][k] in[k]), r < N: 8 lanes per row (consecutive k), 32 rows per pass of the workgroup
template <int K, int N, bool RELU>
__device__ __forceinline__ void block_gemv(const float* __restrict__ W, const float* __restrict__ b, const float* in, float* out, int tid)
{
    constexpr int LPR = 8, ROWS = WG / LPR;
    const int q = tid % LPR;
#pragma unroll
    for (int r0 = 0; r0 < N; r0 += ROWS) {
        const int r = r0 + tid / LPR;
        float acc = 0.0f;
        if (r < N) {
            const float* w = W + (size_t)r * K;
#pragma unroll 8
            for (int k = q; k < K; k += LPR) acc = __fmaf_rn(w[k], in[k], acc);
        }
        acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 1);
        if (q == 0 && r < N) {
            acc += b[r];
            out[r] = RELU ? fmaxf(acc, 0.0f) : acc;
        }
    }
}

// gin[k] = (act[k] > 0) * sum_r W[r][k] g[r], k < 128: thread (k, half) sums half of the rows; `part` is 256 floats of LDS
template <int N>
__device__ __forceinline__ void block_gemv_t(const float* __restrict__ W, const float* g, const float* act, float* part, float* gin, int tid)
{
    const int k = tid & (D_H - 1), half = tid >> 7;
    constexpr int HALF = (N + 1) / 2;
    const int r1 = half ? N : HALF;
    float acc = 0.0f;
    for (int r = half ? HALF : 0; r < r1; r++) acc = __fmaf_rn(W[(size_t)r * D_H + k], g[r], acc);
    part[tid] = acc;
    __syncthreads();
    if (tid < D_H) gin[tid] = act[tid] > 0.0f ? part[tid] + part[tid + D_H] : 0.0f;
    __syncthreads();
}

// dW[r][k] = g[r] in[k], db[r] = g[r]
template <int K, int N>
__device__ __forceinline__ void block_outer(float* __restrict__ dW, float* __restrict__ db, const float* g, const float* in, int tid)
{
    for (int i = tid; i < N * K; i += WG) dW[i] = g[i / K] * in[i % K];
    if (tid < N) db[tid] = g[tid];
}

__global__ void __launch_bounds__(WG)
pose_head_forward_kernel(const moss_pose_head_args a)
{
    __shared__ float s_x[D_IN], s_h1[D_H], s_h2[D_H], s_jf[D_IN], s_S[NJ][3];
    __shared__ int s_par[NJ + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < D_IN) s_x[tid] = a.poses[3 + tid];
    if (tid < NJ + 1) s_par[tid] = a.parents[tid];
    __syncthreads();
    block_gemv<D_IN, D_H, true>(a.params[0], a.params[1], s_x, s_h1, tid);
    __syncthreads();
    block_gemv<D_H, D_H, true>(a.params[2], a.params[3], s_h1, s_h2, tid);
    __syncthreads();
    block_gemv<D_H, D_IN, false>(a.params[4], a.params[5], s_h2, s_jf, tid);
    if (tid < D_H) { a.saved[SV_H1 + tid] = s_h1[tid]; a.saved[SV_H2 + tid] = s_h2[tid]; }
    __syncthreads();
    // the joint layers: thread (j, o) walks j's chain of parents, 3 inputs per node
    float* s_r = s_x;                         // (the poses are not read again)
    if (tid < D_IN) {
        const int j = tid / 3, o = tid % 3;
        const float* w = a.params[6 + 2 * j] + o * a.fc_in[j];
        float acc = a.params[7 + 2 * j][o];
        for (int node = j + 1; node > 0; node = s_par[node], w += 3)
            acc += w[0] * s_jf[3 * node - 3] + w[1] * s_jf[3 * node - 2] + w[2] * s_jf[3 * node - 1];
        a.saved[SV_JF + tid] = s_jf[tid];
        a.saved[SV_R + tid] = acc;
        s_r[tid] = acc;
    }
    __syncthreads();
    if (tid < NJ) {
        float F[9];
        Svd3 d;
        rodrigues(&s_r[3 * tid], F);
        svd3(F, d);
#pragma unroll
        for (int i = 0; i < 9; i++) { a.Rs[9 * tid + i] = F[i]; a.saved[SV_U + 9 * tid + i] = d.U[i]; a.saved[SV_V + 9 * tid + i] = d.V[i]; }
        d.s[2] *= d.det;
#pragma unroll
        for (int i = 0; i < 3; i++) { s_S[tid][i] = d.s[i]; a.S[3 * tid + i] = d.s[i]; }
        a.saved[SV_DET + tid] = d.det;
    }
    __syncthreads();
    for (int j = wave; j < NJ; j += WG / 64) {
        const float S0 = s_S[j][0], S1 = s_S[j][1], S2 = s_S[j][2];
        const float c_bar = wave_integral(S1, S2, S0, false, lane);
        // -<F, target_R>: lanes 0..8 hold one product each (F re-read from Rs: written above by this workgroup, before the barrier)
        float prod = lane < 9 ? a.Rs[9 * j + lane] * a.target_R[9 * j + lane] : 0.0f;
        prod = wave_sum(prod);
        if (lane == 0) {
            a.nll[j] = -prod + a.overreg * (logf(c_bar) + (S0 + S1 + S2));
            a.saved[SV_CBAR + j] = c_bar;
        }
    }
}

__global__ void __launch_bounds__(WG)
pose_head_backward_kernel(const moss_pose_head_backward_args a)
{
    __shared__ float s_x[D_IN], s_h1[D_H], s_h2[D_H], s_jf[D_IN], s_gS[NJ][3], s_dr[D_IN], s_djf[D_IN], s_g2[D_H], s_g1[D_H], s_part[WG];
    __shared__ int s_par[NJ + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < D_IN) { s_x[tid] = a.poses[3 + tid]; s_jf[tid] = a.saved[SV_JF + tid]; }
    if (tid < D_H) { s_h1[tid] = a.saved[SV_H1 + tid]; s_h2[tid] = a.saved[SV_H2 + tid]; }
    if (tid < NJ + 1) s_par[tid] = a.parents[tid];
    // dL/dS_k = g_nll overreg (integral k) / c~
    for (int j = wave; j < NJ; j += WG / 64) {
        const float S[3] = {a.S[3 * j], a.S[3 * j + 1], a.S[3 * j + 2]};
        const float scale = (a.g_nll ? a.g_nll[j] : 0.0f) * a.overreg / a.saved[SV_CBAR + j];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float si, sj, sk;
            shift_args(S, k, si, sj, sk);
            const float v = wave_integral(si, sj, sk, true, lane);
            if (lane == 0) s_gS[j][k] = scale * v;
        }
    }
    __syncthreads();
    if (tid < NJ) {
        const float det = a.saved[SV_DET + tid];
        const float d[3] = {s_gS[tid][0], s_gS[tid][1], s_gS[tid][2] * det};
        float U[9], V[9], G[9], r[3], dr[3];
#pragma unroll
        for (int i = 0; i < 9; i++) { U[i] = a.saved[SV_U + 9 * tid + i]; V[i] = a.saved[SV_V + 9 * tid + i]; }
        u_diag_vt(U, V, d, G);
        const float gn = a.g_nll ? a.g_nll[tid] : 0.0f;
#pragma unroll
        for (int i = 0; i < 9; i++) G[i] += (a.g_Rs ? a.g_Rs[9 * tid + i] : 0.0f) - gn * a.target_R[9 * tid + i];
#pragma unroll
        for (int i = 0; i < 3; i++) r[i] = a.saved[SV_R + 3 * tid + i];
        rodrigues_adjoint(r, G, dr);
#pragma unroll
        for (int i = 0; i < 3; i++) s_dr[3 * tid + i] = dr[i];
    }
    __syncthreads();
    if (tid < D_IN) {
        // weight and bias gradients of the joint layers: thread (j, o) owns row o of fc_pose.j
        const int j = tid / 3, o = tid % 3;
        float* dw = a.grads[6 + 2 * j] + o * a.fc_in[j];
        const float g = s_dr[tid];
        for (int node = j + 1; node > 0; node = s_par[node], dw += 3) {
            dw[0] = g * s_jf[3 * node - 3]; dw[1] = g * s_jf[3 * node - 2]; dw[2] = g * s_jf[3 * node - 1];
        }
        a.grads[7 + 2 * j][o] = g;
    } else if (tid >= D_H && tid < D_H + D_IN) {
        // dL/dh[m][c]: over the joints j, in order, whose chain holds m (at position pos): sum_o fc_j[o][3 pos + c] dr[j][o]
        const int e = tid - D_H, m = e / 3, c = e % 3;
        float acc = 0.0f;
        for (int j = m; j < NJ; j++) {                     // (a chain only holds joints <= its own)
            int pos = 0;
            for (int node = j + 1; node > 0; node = s_par[node], pos++) {
                if (node - 1 == m) {
                    const float* w = a.params[6 + 2 * j] + 3 * pos + c;
                    const int width = a.fc_in[j];
                    acc += w[0] * s_dr[3 * j] + w[width] * s_dr[3 * j + 1] + w[2 * width] * s_dr[3 * j + 2];
                }
            }
        }
        s_djf[e] = acc;
    }
    __syncthreads();
    block_outer<D_H, D_IN>(a.grads[4], a.grads[5], s_djf, s_h2, tid);
    block_gemv_t<D_IN>(a.params[4], s_djf, s_h2, s_part, s_g2, tid);
    block_outer<D_H, D_H>(a.grads[2], a.grads[3], s_g2, s_h1, tid);
    block_gemv_t<D_H>(a.params[2], s_g2, s_h1, s_part, s_g1, tid);
    block_outer<D_IN, D_H>(a.grads[0], a.grads[1], s_g1, s_x, tid);
}

__global__ void __launch_bounds__(WG)
matrix_fisher_nll_kernel(int n, const float* __restrict__ Fm, const float* __restrict__ target, float overreg, float* __restrict__ nll,
                         float* __restrict__ dF)
{
    __shared__ float s_S[NLL_PER_WG][3], s_U[NLL_PER_WG][9], s_V[NLL_PER_WG][9], s_det[NLL_PER_WG], s_gS[NLL_PER_WG][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * NLL_PER_WG, count = min(NLL_PER_WG, n - m0);
    if (tid < count) {
        float F[9];
        Svd3 d;
#pragma unroll
        for (int i = 0; i < 9; i++) F[i] = Fm[9 * (size_t)(m0 + tid) + i];
        svd3(F, d);
#pragma unroll
        for (int i = 0; i < 9; i++) { s_U[tid][i] = d.U[i]; s_V[tid][i] = d.V[i]; }
        s_S[tid][0] = d.s[0]; s_S[tid][1] = d.s[1]; s_S[tid][2] = d.s[2] * d.det;
        s_det[tid] = d.det;
    }
    __syncthreads();
    for (int m = wave; m < count; m += WG / 64) {
        const float S[3] = {s_S[m][0], s_S[m][1], s_S[m][2]};
        const float c_bar = wave_integral(S[1], S[2], S[0], false, lane);
        const size_t o = 9 * (size_t)(m0 + m);
        float prod = lane < 9 ? Fm[o + lane] * target[o + lane] : 0.0f;
        prod = wave_sum(prod);
        if (lane == 0) nll[m0 + m] = -prod + overreg * (logf(c_bar) + (S[0] + S[1] + S[2]));
        if (dF) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float si, sj, sk;
                shift_args(S, k, si, sj, sk);
                const float v = wave_integral(si, sj, sk, true, lane);
                if (lane == 0) s_gS[m][k] = overreg * v / c_bar;
            }
        }
    }
    if (!dF) return;
    __syncthreads();
    if (tid < count) {
        const float d[3] = {s_gS[tid][0], s_gS[tid][1], s_gS[tid][2] * s_det[tid]};
        float G[9];
        u_diag_vt(s_U[tid], s_V[tid], d, G);
        const size_t o = 9 * (size_t)(m0 + tid);
#pragma unroll
        for (int i = 0; i < 9; i++) dF[o + i] = G[i] - target[o + i];
    }
}

// the checks both directions share; `who` prefixes the message
template <typename A>
int pose_check(const A* a, const char* who)
{
    const char* const null_msg = "null argument block, poses, target_R or parameter";
    const char* const parents_msg = "parents[0] must be -1 and 0 <= parents[i] < i";
    if (!a || !a->poses || !a->target_R) return invalid_arg(who, null_msg);
    for (int i = 0; i < NP; i++)
        if (!a->params[i]) return invalid_arg(who, null_msg);
    if (a->parents[0] != -1) return invalid_arg(who, parents_msg);
    for (int i = 1; i <= NJ; i++)
        if (a->parents[i] < 0 || a->parents[i] >= i) return invalid_arg(who, parents_msg);
    for (int j = 0; j < NJ; j++) {
        int nodes = 0;
        for (int node = j + 1; node > 0; node = a->parents[node]) nodes++;
        if (a->fc_in[j] != 3 * nodes) return invalid_arg(who, "fc_in[j] must be 3 * (1 + the number of non-root ancestors of joint j)");
    }
    return 0;
}

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" int moss_pose_head_forward(const moss_pose_head_args* a, void* stream)
{
    if (int rc = pose_check(a, "moss_pose_head_forward")) return rc;
    if (!a->Rs || !a->S || !a->nll || !a->saved) return invalid_arg("moss_pose_head_forward", "null output (Rs, S, nll, saved)");
    hipLaunchKernelGGL(pose_head_forward_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, *a);
    return launch_status("moss_pose_head_forward");
}

extern "C" int moss_pose_head_backward(const moss_pose_head_backward_args* a, void* stream)
{
    if (int rc = pose_check(a, "moss_pose_head_backward")) return rc;
    if (!a->S || !a->saved) return invalid_arg("moss_pose_head_backward", "null S or saved (the forward's)");
    for (int i = 0; i < NP; i++)
        if (!a->grads[i]) return invalid_arg("moss_pose_head_backward", "null gradient tensor (all 52 are written)");
    hipLaunchKernelGGL(pose_head_backward_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, *a);
    return launch_status("moss_pose_head_backward");
}

extern "C" int moss_matrix_fisher_nll(int n, const float* F, const float* target_R, float overreg, float* nll_out, float* dF_out,
                                      void* stream)
{
    if (n < 0) return invalid_arg("moss_matrix_fisher_nll", "n must be >= 0");
    if (n == 0) return 0;
    if (!F || !target_R || !nll_out) return invalid_arg("moss_matrix_fisher_nll", "null F, target_R or nll_out");
    hipLaunchKernelGGL(matrix_fisher_nll_kernel, dim3((n + NLL_PER_WG - 1) / NLL_PER_WG), dim3(WG), 0, (hipStream_t)stream, n, F,
                       target_R, overreg, nll_out, dF_out);
    return launch_status("moss_matrix_fisher_nll");
}
