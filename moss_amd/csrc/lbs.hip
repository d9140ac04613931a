// lbs.hip -- per-Gaussian linear blend skinning of MOSS's coarse_deform_c2source (include/moss_raster.h moss_lbs_deform_forward /
// moss_lbs_deform_backward; the formulas are restated there).
//
// forward:  one lane per Gaussian.  The J x 12 floats of A_big and A_obs (rows 0..2 of each 4x4) and R, Th are wave-uniform: each
//           workgroup reads them once into LDS, and every lane reads them back as broadcast ds_read_b128.  The lane blends its two
//           3x4 matrices from its weights, inverts the 3x3 block by adjugate and determinant and writes T, t (+ p, w).
// backward: one lane per Gaussian, the forward recomputed, then the hand-derived adjoint (moss_amd/lbs.py deform_torch is the same
//           math in torch).  The J x 12 gradient of A_obs is sum_i w_ij gO_i: each workgroup of 128 lanes stages w and gO in LDS and
//           forms its 128-term sums in a fixed order (one output element per thread), the J x 12 partials of every workgroup go to
//           the workspace, and a fold launch adds them up in workgroup order in float64.  No atomics: bitwise reproducible.
// backward_frame (moss_lbs_deform_backward_frame): the backward kernel as it is (so its outputs keep their bits), and beside it a
//           kernel of the same shape that forms, per Gaussian, the twelve terms of g_R = sum_i (gT'_i N_i^T + gt'_i n_i^T) and
//           g_Th = sum_i gt'_i (N = O3 Q, n = O3 (d - Q b) + o).  They ride the same reduction: staged in LDS, summed per workgroup
//           in lane order in float64 (one value per thread), folded in workgroup order by the same fold launch.  Every loop's trip
//           count is a constant or the number of workgroups.
// Instantiations: J = 24 (SMPL) with 16-byte loads and stores of the W / L / w rows, and J rounded up to a multiple of 8 (8 .. 64)
// with per-element guards for every other J.  Nothing is allocated, nothing synchronises, nothing is cleared with a memset.
#include "common.h"
#include "wave.h"

namespace moss {

namespace {

constexpr int LBS_FWD_BLOCK = 256;
constexpr int LBS_BWD_BLOCK = 128;
constexpr int LBS_MAX_J = MOSS_SMPL_FRAME_MAX_JOINTS;
constexpr int LBS_FOLD_WAVES = 4;

struct LbsIn {
    int P, J, V;
    const int64_t* ids;
    const float* W;
    const float* L;
    const float* Abig;
    const float* Aobs;
    const float* d;
    const float* R;
    const float* Th;
    const float* x;
};

// rows 0..2 of every A[j] as float4 (s_A[3 j + r]); R row-major in s_RT[0..8], Th in s_RT[9..11]
__device__ __forceinline__ void lbs_stage_frame(const LbsIn& a, float4* s_Ab, float4* s_Ao, float* s_RT)
{
    for (int k = threadIdx.x; k < a.J * 3; k += blockDim.x) {
        const int j = k / 3, r = k % 3;
        const float* pb = a.Abig + j * 16 + r * 4;
        const float* po = a.Aobs + j * 16 + r * 4;
        s_Ab[k] = make_float4(pb[0], pb[1], pb[2], pb[3]);
        s_Ao[k] = make_float4(po[0], po[1], po[2], po[3]);
    }
    if (threadIdx.x < 12) s_RT[threadIdx.x] = threadIdx.x < 9 ? a.R[threadIdx.x] : a.Th[threadIdx.x - 9];
}

template <int JB, bool VEC>
__device__ __forceinline__ void lbs_load_row(const float* row, int J, float (&v)[JB])
{
    if (VEC) {
#pragma unroll
        for (int q = 0; q < JB / 4; q++) {
            const float4 f = reinterpret_cast<const float4*>(row)[q];
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < JB; j++) v[j] = j < J ? row[j] : 0.0f;
    }
}

template <int JB, bool VEC>
__device__ __forceinline__ void lbs_write_row(float* row, int J, const float (&v)[JB])
{
    if (VEC) {
#pragma unroll
        for (int q = 0; q < JB / 4; q++)
            reinterpret_cast<float4*>(row)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < JB; j++)
            if (j < J) row[j] = v[j];
    }
}

// the blend weights of Gaussian i with vertex v: W[v], or softmax(log(W[v] + 1e-9) + L[i]) as torch's F.softmax forms it
// (max, exp(z - max), sum, divide).  Entries j >= J are zero.
template <int JB, bool VEC>
__device__ __forceinline__ void lbs_weights(const LbsIn& a, int i, int64_t v, float (&w)[JB])
{
    lbs_load_row<JB, VEC>(a.W + (size_t)v * a.J, a.J, w);
    if (a.L) {
        float l[JB];
        lbs_load_row<JB, VEC>(a.L + (size_t)i * a.J, a.J, l);
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < JB; j++)
            if (j < a.J) { l[j] = logf(w[j] + 1e-9f) + l[j]; m = fmaxf(m, l[j]); }
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < JB; j++)
            if (j < a.J) { l[j] = expf(l[j] - m); s += l[j]; }
#pragma unroll
        for (int j = 0; j < JB; j++) w[j] = j < a.J ? l[j] / s : 0.0f;
    }
}

// everything the forward forms per Gaussian (the backward needs all of it)
struct LbsState {
    float B[12], O[12];     // the blended 3x4 matrices [B3 | b], [O3 | o], row-major
    float Q[9], M[9], T[9]; // B3^-1, R O3, M Q
    float u[3];             // d - Q b
    float t[3];
};

template <int JB>
__device__ __forceinline__ void lbs_state(const float (&w)[JB], int J, const float4* s_Ab, const float4* s_Ao, const float* s_RT,
                                          const float* d, LbsState& s)
{
#pragma unroll
    for (int k = 0; k < 12; k++) { s.B[k] = 0.0f; s.O[k] = 0.0f; }
#pragma unroll
    for (int j = 0; j < JB; j++) {
        if (j < J) {
            const float wj = w[j];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const float4 ab = s_Ab[3 * j + r], ao = s_Ao[3 * j + r];
                s.B[4 * r] = fmaf(wj, ab.x, s.B[4 * r]); s.B[4 * r + 1] = fmaf(wj, ab.y, s.B[4 * r + 1]);
                s.B[4 * r + 2] = fmaf(wj, ab.z, s.B[4 * r + 2]); s.B[4 * r + 3] = fmaf(wj, ab.w, s.B[4 * r + 3]);
                s.O[4 * r] = fmaf(wj, ao.x, s.O[4 * r]); s.O[4 * r + 1] = fmaf(wj, ao.y, s.O[4 * r + 1]);
                s.O[4 * r + 2] = fmaf(wj, ao.z, s.O[4 * r + 2]); s.O[4 * r + 3] = fmaf(wj, ao.w, s.O[4 * r + 3]);
            }
        }
    }
    const float b00 = s.B[0], b01 = s.B[1], b02 = s.B[2], b10 = s.B[4], b11 = s.B[5], b12 = s.B[6];
    const float b20 = s.B[8], b21 = s.B[9], b22 = s.B[10];
    const float c00 = b11 * b22 - b12 * b21, c01 = b02 * b21 - b01 * b22, c02 = b01 * b12 - b02 * b11;
    const float c10 = b12 * b20 - b10 * b22, c11 = b00 * b22 - b02 * b20, c12 = b02 * b10 - b00 * b12;
    const float c20 = b10 * b21 - b11 * b20, c21 = b01 * b20 - b00 * b21, c22 = b00 * b11 - b01 * b10;
    const float inv = 1.0f / (b00 * c00 + b01 * c10 + b02 * c20);     // a singular B3: inf, and the rows go inf / NaN
    s.Q[0] = c00 * inv; s.Q[1] = c01 * inv; s.Q[2] = c02 * inv;
    s.Q[3] = c10 * inv; s.Q[4] = c11 * inv; s.Q[5] = c12 * inv;
    s.Q[6] = c20 * inv; s.Q[7] = c21 * inv; s.Q[8] = c22 * inv;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            s.M[3 * r + c] = s_RT[3 * r] * s.O[c] + s_RT[3 * r + 1] * s.O[4 + c] + s_RT[3 * r + 2] * s.O[8 + c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            s.T[3 * r + c] = s.M[3 * r] * s.Q[c] + s.M[3 * r + 1] * s.Q[3 + c] + s.M[3 * r + 2] * s.Q[6 + c];
#pragma unroll
    for (int r = 0; r < 3; r++)
        s.u[r] = d[r] - (s.Q[3 * r] * s.B[3] + s.Q[3 * r + 1] * s.B[7] + s.Q[3 * r + 2] * s.B[11]);
#pragma unroll
    for (int r = 0; r < 3; r++)
        s.t[r] = (s.M[3 * r] * s.u[0] + s.M[3 * r + 1] * s.u[1] + s.M[3 * r + 2] * s.u[2])
               + (s_RT[3 * r] * s.O[3] + s_RT[3 * r + 1] * s.O[7] + s_RT[3 * r + 2] * s.O[11]) + s_RT[9 + r];
}

template <int JB, bool VEC>
__global__ void __launch_bounds__(LBS_FWD_BLOCK)
lbs_forward_kernel(LbsIn a, float* __restrict__ outT, float* __restrict__ outt, float* __restrict__ outp, float* __restrict__ outw)
{
    __shared__ float4 s_Ab[3 * JB], s_Ao[3 * JB];
    __shared__ float s_RT[12];
    lbs_stage_frame(a, s_Ab, s_Ao, s_RT);
    __syncthreads();
    const int i = blockIdx.x * LBS_FWD_BLOCK + threadIdx.x;
    if (i >= a.P) return;
    const int64_t v = a.ids[i];
    if (v < 0 || v >= a.V) {                                   // never dereferenced: NaN rows
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 9; k++) outT[(size_t)i * 9 + k] = nan;
#pragma unroll
        for (int k = 0; k < 3; k++) outt[(size_t)i * 3 + k] = nan;
        if (outp) {
#pragma unroll
            for (int k = 0; k < 3; k++) outp[(size_t)i * 3 + k] = nan;
        }
        if (outw) for (int j = 0; j < a.J; j++) outw[(size_t)i * a.J + j] = nan;
        return;
    }
    float w[JB];
    lbs_weights<JB, VEC>(a, i, v, w);
    LbsState s;
    lbs_state<JB>(w, a.J, s_Ab, s_Ao, s_RT, a.d + (size_t)i * 3, s);
#pragma unroll
    for (int k = 0; k < 9; k++) outT[(size_t)i * 9 + k] = s.T[k];
#pragma unroll
    for (int k = 0; k < 3; k++) outt[(size_t)i * 3 + k] = s.t[k];
    if (outp) {
        const float* x = a.x + (size_t)i * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
        for (int r = 0; r < 3; r++) outp[(size_t)i * 3 + r] = (s.T[3 * r] * x0 + s.T[3 * r + 1] * x1 + s.T[3 * r + 2] * x2) + s.t[r];
    }
    if (outw) lbs_write_row<JB, VEC>(outw + (size_t)i * a.J, a.J, w);
}

struct LbsGrad {
    const float* gT; const float* gt; const float* gp;
    float* gL; float* gd; float* gx;
    float* partials;        // [blocks][J][12], or NULL: no gradient of A_obs
};

template <int JB, bool VEC>
__global__ void __launch_bounds__(LBS_BWD_BLOCK)
lbs_backward_kernel(LbsIn a, LbsGrad g)
{
    __shared__ float4 s_Ab[3 * JB], s_Ao[3 * JB];
    __shared__ float s_RT[12];
    __shared__ float s_w[LBS_BWD_BLOCK][JB];                // this workgroup's weights and [gO3 | go], for the A_obs reduction
    __shared__ float s_g[LBS_BWD_BLOCK][12];
    lbs_stage_frame(a, s_Ab, s_Ao, s_RT);
    __syncthreads();
    const int lane = threadIdx.x;
    const int i = blockIdx.x * LBS_BWD_BLOCK + lane;
    const int64_t v = i < a.P ? a.ids[i] : 0;
    const bool valid = i < a.P && v >= 0 && v < a.V;
    float w[JB], gO[12];
#pragma unroll
    for (int j = 0; j < JB; j++) w[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; k++) gO[k] = 0.0f;
    if (valid) {
        lbs_weights<JB, VEC>(a, i, v, w);
        LbsState s;
        lbs_state<JB>(w, a.J, s_Ab, s_Ao, s_RT, a.d + (size_t)i * 3, s);
        const float* R = s_RT;
        float gT[9], gt[3], gp[3], x[3];
#pragma unroll
        for (int k = 0; k < 9; k++) gT[k] = g.gT ? g.gT[(size_t)i * 9 + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gt[k] = g.gt ? g.gt[(size_t)i * 3 + k] : 0.0f;
            gp[k] = g.gp ? g.gp[(size_t)i * 3 + k] : 0.0f;
            x[k] = a.x ? a.x[(size_t)i * 3 + k] : 0.0f;
        }
        // p = T x + t:  gT' = gT + gp x^T, gt' = gt + gp, gx = T^T gp
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) gT[3 * r + c] = fmaf(gp[r], x[c], gT[3 * r + c]);
            gt[r] += gp[r];
        }
        if (g.gx) {
#pragma unroll
            for (int c = 0; c < 3; c++) g.gx[(size_t)i * 3 + c] = s.T[c] * gp[0] + s.T[3 + c] * gp[1] + s.T[6 + c] * gp[2];
        }
        // T = M Q, t = M u + R o + Th, u = d - Q b:  gM = gT Q^T + gt u^T;  gQ = M^T (gT - gt b^T);  gd = M^T gt
        const float b[3] = {s.B[3], s.B[7], s.B[11]};
        float gM[9], gQ[9], gd[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)
                gM[3 * r + c] = gT[3 * r] * s.Q[3 * c] + gT[3 * r + 1] * s.Q[3 * c + 1] + gT[3 * r + 2] * s.Q[3 * c + 2] + gt[r] * s.u[c];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)
                gQ[3 * r + c] = s.M[r] * (gT[c] - gt[0] * b[c]) + s.M[3 + r] * (gT[3 + c] - gt[1] * b[c])
                              + s.M[6 + r] * (gT[6 + c] - gt[2] * b[c]);
#pragma unroll
        for (int c = 0; c < 3; c++) gd[c] = s.M[c] * gt[0] + s.M[3 + c] * gt[1] + s.M[6 + c] * gt[2];
        if (g.gd) {
#pragma unroll
            for (int c = 0; c < 3; c++) g.gd[(size_t)i * 3 + c] = gd[c];
        }
        // M = R O3, the R o term:  gO3 = R^T gM, go = R^T gt
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) gO[4 * r + c] = R[r] * gM[c] + R[3 + r] * gM[3 + c] + R[6 + r] * gM[6 + c];
            gO[4 * r + 3] = R[r] * gt[0] + R[3 + r] * gt[1] + R[6 + r] * gt[2];
        }
        // Q = B3^-1:  gB3 = -Q^T gQ Q^T;  b enters through u only:  gb = -Q^T gd = -T^T gt (gd = M^T gt)
        float gB[12], X[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)                                                    // X = Q^T gQ
                X[3 * r + c] = s.Q[r] * gQ[c] + s.Q[3 + r] * gQ[3 + c] + s.Q[6 + r] * gQ[6 + c];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++)                                                    // -X Q^T
                gB[4 * r + c] = -(X[3 * r] * s.Q[3 * c] + X[3 * r + 1] * s.Q[3 * c + 1] + X[3 * r + 2] * s.Q[3 * c + 2]);
            gB[4 * r + 3] = -(s.Q[r] * gd[0] + s.Q[3 + r] * gd[1] + s.Q[6 + r] * gd[2]);
        }
        if (g.gL) {
            // gw_j = <gO, A_obs[j]> + <gB, A_big[j]>;  softmax:  gL = w (gw - <w, gw>)
            float gw[JB];
            float sw = 0.0f;
#pragma unroll
            for (int j = 0; j < JB; j++) {
                float acc = 0.0f;
                if (j < a.J) {
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const float4 ab = s_Ab[3 * j + r], ao = s_Ao[3 * j + r];
                        acc = fmaf(gO[4 * r], ao.x, acc); acc = fmaf(gO[4 * r + 1], ao.y, acc);
                        acc = fmaf(gO[4 * r + 2], ao.z, acc); acc = fmaf(gO[4 * r + 3], ao.w, acc);
                        acc = fmaf(gB[4 * r], ab.x, acc); acc = fmaf(gB[4 * r + 1], ab.y, acc);
                        acc = fmaf(gB[4 * r + 2], ab.z, acc); acc = fmaf(gB[4 * r + 3], ab.w, acc);
                    }
                }
                gw[j] = acc;
                sw = fmaf(w[j], acc, sw);
            }
#pragma unroll
            for (int j = 0; j < JB; j++) gw[j] = w[j] * (gw[j] - sw);
            lbs_write_row<JB, VEC>(g.gL + (size_t)i * a.J, a.J, gw);
        }
    } else if (i < a.P) {                                      // out-of-range id: NaN rows, nothing into the reduction
        const float nan = __builtin_nanf("");
        if (g.gd) for (int c = 0; c < 3; c++) g.gd[(size_t)i * 3 + c] = nan;
        if (g.gx) for (int c = 0; c < 3; c++) g.gx[(size_t)i * 3 + c] = nan;
        if (g.gL) for (int j = 0; j < a.J; j++) g.gL[(size_t)i * a.J + j] = nan;
    }
    if (!g.partials) return;                                   // (uniform over the launch)
    // this workgroup's share of gA_obs[j] = sum_i w_ij gO_i: lanes past P and invalid ids staged zeros above
#pragma unroll
    for (int j = 0; j < JB; j++) s_w[lane][j] = w[j];
#pragma unroll
    for (int k = 0; k < 12; k++) s_g[lane][k] = gO[k];
    __syncthreads();
    const int nout = a.J * 12;
    float* part = g.partials + (size_t)blockIdx.x * nout;
    for (int o = lane; o < nout; o += LBS_BWD_BLOCK) {
        const int k = o / a.J, j = o % a.J;                   // consecutive lanes: consecutive j (s_w conflict-free), one k (broadcast)
        float acc = 0.0f;
#pragma unroll 8
        for (int q = 0; q < LBS_BWD_BLOCK; q++) acc = fmaf(s_w[q][j], s_g[q][k], acc);
        part[j * 12 + k] = acc;
    }
}

// this workgroup's share of [g_R | g_Th]: one lane per Gaussian (the workgroups of lbs_backward_kernel), the forward recomputed;
// fpartials [blocks][12] (g_R row-major, then g_Th).  Lanes past P and Gaussians with an id outside [0, V) stage zeros.
template <int JB, bool VEC>
__global__ void __launch_bounds__(LBS_BWD_BLOCK)
lbs_frame_terms_kernel(LbsIn a, const float* __restrict__ g_T, const float* __restrict__ g_t, const float* __restrict__ g_p,
                       double* __restrict__ fpartials)
{
    __shared__ float4 s_Ab[3 * JB], s_Ao[3 * JB];
    __shared__ float s_RT[12];
    __shared__ float s_f[LBS_BWD_BLOCK][12];
    lbs_stage_frame(a, s_Ab, s_Ao, s_RT);
    __syncthreads();
    const int lane = threadIdx.x;
    const int i = blockIdx.x * LBS_BWD_BLOCK + lane;
    const int64_t v = i < a.P ? a.ids[i] : 0;
    const bool valid = i < a.P && v >= 0 && v < a.V;
    float gF[12];
#pragma unroll
    for (int k = 0; k < 12; k++) gF[k] = 0.0f;
    if (valid) {
        float w[JB];
        lbs_weights<JB, VEC>(a, i, v, w);
        LbsState s;
        lbs_state<JB>(w, a.J, s_Ab, s_Ao, s_RT, a.d + (size_t)i * 3, s);
        float gT[9], gt[3], gp[3], x[3];
#pragma unroll
        for (int k = 0; k < 9; k++) gT[k] = g_T ? g_T[(size_t)i * 9 + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gt[k] = g_t ? g_t[(size_t)i * 3 + k] : 0.0f;
            gp[k] = g_p ? g_p[(size_t)i * 3 + k] : 0.0f;
            x[k] = a.x ? a.x[(size_t)i * 3 + k] : 0.0f;
        }
        // p = T x + t:  gT' = gT + gp x^T, gt' = gt + gp
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) gT[3 * r + c] = fmaf(gp[r], x[c], gT[3 * r + c]);
            gt[r] += gp[r];
        }
        // T = R N, t = R n + Th with N = O3 Q, n = O3 u + o:  gR = gT' N^T + gt' n^T;  gTh = gt'
        float N[9], n[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                N[3 * r + c] = s.O[4 * r] * s.Q[c] + s.O[4 * r + 1] * s.Q[3 + c] + s.O[4 * r + 2] * s.Q[6 + c];
            n[r] = (s.O[4 * r] * s.u[0] + s.O[4 * r + 1] * s.u[1] + s.O[4 * r + 2] * s.u[2]) + s.O[4 * r + 3];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                gF[3 * r + c] = gT[3 * r] * N[3 * c] + gT[3 * r + 1] * N[3 * c + 1] + gT[3 * r + 2] * N[3 * c + 2] + gt[r] * n[c];
            gF[9 + r] = gt[r];
        }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) s_f[lane][k] = gF[k];
    __syncthreads();
    if (lane < 12) {
        double acc = 0.0;
#pragma unroll 8
        for (int q = 0; q < LBS_BWD_BLOCK; q++) acc += (double)s_f[q][lane];
        fpartials[(size_t)blockIdx.x * 12 + lane] = acc;
    }
}

// the fold of both backwards, one wave per element: the workgroup partials in workgroup order (lane l takes l, l + 64, ...) in float64,
// then a fixed butterfly.  Elements [0, 16 J) are gA_obs (J,4,4), row 3 of every 4x4 written as zero (skipped without gA); elements
// 16 J + [0, 12) are [g_R | g_Th] from the float64 partials (moss_lbs_deform_backward's grid ends before them).  nblocks = 0 (P = 0)
// writes zeros.
__global__ void __launch_bounds__(64 * LBS_FOLD_WAVES)
lbs_fold_kernel(int J, int nblocks, const float* __restrict__ partials, float* __restrict__ gA,
                      const double* __restrict__ fpartials, float* __restrict__ gR, float* __restrict__ gTh)
{
    const int o = blockIdx.x * LBS_FOLD_WAVES + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (o >= J * 16 + 12) return;
    double acc = 0.0;
    if (o < J * 16) {
        if (!gA) return;
        const int j = o / 16, r = (o % 16) / 4, c = o % 4;
        if (r < 3) {
            const size_t stride = (size_t)J * 12, off = (size_t)j * 12 + r * 4 + c;
            for (int b = lane; b < nblocks; b += 64) acc += (double)partials[(size_t)b * stride + off];
        }
        acc = wave_sum(acc);
        if (lane == 0) gA[o] = (float)acc;
        return;
    }
    const int k = o - J * 16;
    float* out = k < 9 ? (gR ? gR + k : nullptr) : (gTh ? gTh + (k - 9) : nullptr);
    if (!out) return;
    for (int b = lane; b < nblocks; b += 64) acc += fpartials[(size_t)b * 12 + k];
    acc = wave_sum(acc);
    if (lane == 0) *out = (float)acc;
}

// the instantiation for J: 24 with 16-byte row accesses when the rows are 16-byte aligned, else J rounded up to a multiple of 8
template <template <int, bool> class F, typename... Args>
void lbs_dispatch(int J, bool vec, Args... args)
{
    if (J == 24 && vec) { F<24, true>::run(args...); return; }
    switch ((J + 7) / 8) {
    case 1: F<8, false>::run(args...); break;
    case 2: F<16, false>::run(args...); break;
    case 3: F<24, false>::run(args...); break;
    case 4: F<32, false>::run(args...); break;
    case 5: F<40, false>::run(args...); break;
    case 6: F<48, false>::run(args...); break;
    case 7: F<56, false>::run(args...); break;
    default: F<64, false>::run(args...); break;
    }
}

template <int JB, bool VEC>
struct LaunchFwd {
    static void run(dim3 grid, hipStream_t s, LbsIn a, float* T, float* t, float* p, float* w)
    {
        hipLaunchKernelGGL((lbs_forward_kernel<JB, VEC>), grid, dim3(LBS_FWD_BLOCK), 0, s, a, T, t, p, w);
    }
};

template <int JB, bool VEC>
struct LaunchBwd {
    static void run(dim3 grid, hipStream_t s, LbsIn a, LbsGrad g)
    {
        hipLaunchKernelGGL((lbs_backward_kernel<JB, VEC>), grid, dim3(LBS_BWD_BLOCK), 0, s, a, g);
    }
};

template <int JB, bool VEC>
struct LaunchFrameTerms {
    static void run(dim3 grid, hipStream_t s, LbsIn a, const float* gT, const float* gt, const float* gp, double* fpartials)
    {
        hipLaunchKernelGGL((lbs_frame_terms_kernel<JB, VEC>), grid, dim3(LBS_BWD_BLOCK), 0, s, a, gT, gt, gp, fpartials);
    }
};

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename A>
int lbs_check_common(const char* who, const A* a)
{
    if (!a) return invalid_arg(who, "null argument block");
    if (a->P < 0) return invalid_arg(who, "P must be >= 0");
    if (a->J < 1 || a->J > LBS_MAX_J) return invalid_arg(who, "J must be 1..64");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (!a->vert_ids || !a->weights || !a->A_big || !a->A_obs || !a->d || !a->R || !a->Th)
        return invalid_arg(who, "null required input (vert_ids, weights, A_big, A_obs, d, R, Th)");
    return 0;
}

template <typename A>
LbsIn lbs_in(const A* a)
{
    return LbsIn{a->P, a->J, a->V, a->vert_ids, a->weights, a->lbs_offsets, a->A_big, a->A_obs, a->d, a->R, a->Th, a->x};
}

// both backward entries.  FRAME (moss_lbs_deform_backward_frame): the block also has g_R and g_Th, the workspace rule is
// moss_lbs_frame_workspace_bytes, the texts carry the entry's full name, and P = 0 still writes zero g_R / g_Th; the plain entry
// returns at P = 0 before it looks at the workspace, launches its kernel whatever is wanted, and folds gA_obs's elements alone.
template <bool FRAME, typename A>
int lbs_backward_impl(const A* a, void* stream)
{
    const char* entry = FRAME ? "moss_lbs_deform_backward_frame" : "moss_lbs_deform_backward";
    const char* who = FRAME ? entry : "lbs backward";
    if (int rc = lbs_check_common(FRAME ? entry : "lbs", a)) return rc;
    if ((a->g_p || a->g_x) && !a->x) return invalid_arg(who, "g_p and g_x need x");
    if (a->g_L && !a->lbs_offsets) return invalid_arg(who, "g_L needs lbs_offsets");
    float* g_R = nullptr;
    float* g_Th = nullptr;
    if constexpr (FRAME) { g_R = a->g_R; g_Th = a->g_Th; }
    else if (a->P == 0) return 0;
    const bool frame = g_R || g_Th;
    if (a->P > 0 && (a->g_A_obs || frame)
        && (!a->workspace || a->workspace_bytes < (FRAME ? moss_lbs_frame_workspace_bytes : moss_lbs_workspace_bytes)(a->P, a->J)))
        return invalid_arg(who, FRAME ? "g_A_obs, g_R and g_Th need moss_lbs_frame_workspace_bytes(P, J) bytes of workspace"
                                      : "g_A_obs needs moss_lbs_workspace_bytes(P, J) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (a->P + LBS_BWD_BLOCK - 1) / LBS_BWD_BLOCK;
    float* partials = nullptr;
    double* fpartials = nullptr;
    if (a->P > 0) {
        partials = a->g_A_obs ? reinterpret_cast<float*>(a->workspace) : nullptr;
        fpartials = frame ? reinterpret_cast<double*>(a->workspace + moss_lbs_workspace_bytes(a->P, a->J)) : nullptr;
        const bool vec = aligned16(a->weights) && aligned16(a->lbs_offsets) && aligned16(a->g_L);
        if (!FRAME || a->g_L || a->g_A_obs || a->g_d || a->g_x) {
            const LbsGrad g{a->g_T, a->g_t, a->g_p, a->g_L, a->g_d, a->g_x, partials};
            lbs_dispatch<LaunchBwd>(a->J, vec, dim3(nblocks), s, lbs_in(a), g);
        }
        if (frame) lbs_dispatch<LaunchFrameTerms>(a->J, vec, dim3(nblocks), s, lbs_in(a), a->g_T, a->g_t, a->g_p, fpartials);
    }
    // P = 0: nothing reads a Gaussian; g_R and g_Th are written as zero (g_A_obs is not written)
    float* gA = a->P > 0 ? a->g_A_obs : nullptr;
    if (gA || frame)
        hipLaunchKernelGGL(lbs_fold_kernel, dim3((a->J * 16 + (FRAME ? 12 : 0) + LBS_FOLD_WAVES - 1) / LBS_FOLD_WAVES),
                           dim3(64 * LBS_FOLD_WAVES), 0, s, a->J, nblocks, (const float*)partials, gA, (const double*)fpartials, g_R, g_Th);
    return launch_status(entry);
}

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_lbs_workspace_bytes(int P, int J)
{
    if (P <= 0 || J < 1 || J > LBS_MAX_J) return 0;
    const size_t nb = ((size_t)P + LBS_BWD_BLOCK - 1) / LBS_BWD_BLOCK;
    return align_up(nb * (size_t)J * 12 * sizeof(float));
}

extern "C" int moss_lbs_deform_forward(const moss_lbs_forward_args* a, void* stream)
{
    if (int rc = lbs_check_common("lbs", a)) return rc;
    if (!a->T || !a->t) return invalid_arg("lbs forward", "null T or t");
    if (a->p && !a->x) return invalid_arg("lbs forward", "p needs x");
    if (a->P == 0) return 0;
    const bool vec = aligned16(a->weights) && aligned16(a->lbs_offsets) && aligned16(a->w);
    const dim3 grid((a->P + LBS_FWD_BLOCK - 1) / LBS_FWD_BLOCK);
    lbs_dispatch<LaunchFwd>(a->J, vec, grid, (hipStream_t)stream, lbs_in(a), a->T, a->t, a->p, a->w);
    return launch_status("moss_lbs_deform_forward");
}

extern "C" size_t moss_lbs_frame_workspace_bytes(int P, int J)
{
    if (P <= 0 || J < 1 || J > LBS_MAX_J) return 0;
    const size_t nb = ((size_t)P + LBS_BWD_BLOCK - 1) / LBS_BWD_BLOCK;
    return moss_lbs_workspace_bytes(P, J) + align_up(nb * 12 * sizeof(double));
}

extern "C" int moss_lbs_deform_backward(const moss_lbs_backward_args* a, void* stream) { return lbs_backward_impl<false>(a, stream); }

extern "C" int moss_lbs_deform_backward_frame(const moss_lbs_backward_frame_args* a, void* stream)
{
    return lbs_backward_impl<true>(a, stream);
}
