// smpl_math.h -- what the per-frame SMPL kernels (smpl_frame.hip, frame_bounds.hip) share: Rodrigues and its adjoint, the parents table and its check,
// and the steps of the skeleton that both files take -- the shaped template and regressor shares of a range of vertices, its
// pose-blend rows, the fold of the shares into joints, the relative joints, a step of the chain and an entry of A.  The steps are
// templated on S, the number of shape sets a kernel carries: 2 in smpl_frame.hip (the big pose's, the frame's), 1 in frame_bounds.hip.
// Every sum is float64 in a fixed order; the LDS arrays belong to the kernels.
#pragma once
#include "common.h"
#include "wave.h"

namespace moss {

constexpr int SMPL_MAX_J = MOSS_SMPL_FRAME_MAX_JOINTS;
constexpr int SMPL_MAX_F = 9 * (SMPL_MAX_J - 1);
constexpr int SMPL_VPB = 16;              // vertices per workgroup of the kernels that stream posedirs (offsets, posed)

struct SmplParents { int32_t p[SMPL_MAX_J]; };

template <typename A>
inline SmplParents smpl_parents(const A* a)
{
    SmplParents par;
    for (int j = 0; j < SMPL_MAX_J; j++) par.p[j] = j < a->J ? a->parents[j] : 0;
    return par;
}

inline int smpl_check_parents(const char* who, int J, const int32_t* parents)
{
    for (int j = 1; j < J; j++)
        if (parents[j] < 0 || parents[j] >= j) return invalid_arg(who, "parents[j] must be in [0, j) for every j >= 1");
    return 0;
}

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

// the adjoint of r -> raw = I + s K + c K K, e = r + 1e-8, a = |e|, k = r / a, s = sin a, c = 1 - cos a (K K = k k^T - |k|^2 I; the
// shift is in the norm only), for the cotangent G of raw:
//   g_s = <G, K>, g_c = <G, K K>, gK = s G + c (G K^T + K^T G), g_k = (gK_21 - gK_12, gK_02 - gK_20, gK_10 - gK_01),
//   g_a = g_s cos a + g_c sin a - <g_k, r> / a^2,  g_r = g_k / a + g_a e / a.
__device__ __forceinline__ void smpl_rodrigues_adjoint(const double* G, const float* r, float* g_r)
{
    const double rx = (double)r[0], ry = (double)r[1], rz = (double)r[2];
    const double ex = rx + 1e-8, ey = ry + 1e-8, ez = rz + 1e-8;
    const double a = sqrt(ex * ex + ey * ey + ez * ez);
    const double kx = rx / a, ky = ry / a, kz = rz / a;
    const double sh = sin(0.5 * a), sn = sin(a), cs = cos(a);
    const double cc = 2.0 * sh * sh;                           // 1 - cos a, without the cancellation at small angles
    const double K[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
    const double kk = kx * kx + ky * ky + kz * kz;
    const double KK[9] = {kx * kx - kk, kx * ky, kx * kz, kx * ky, ky * ky - kk, ky * kz, kx * kz, ky * kz, kz * kz - kk};
    double g_s = 0.0, g_c = 0.0;
#pragma unroll
    for (int e = 0; e < 9; e++) { g_s = fma(G[e], K[e], g_s); g_c = fma(G[e], KK[e], g_c); }
    double gK[9];
#pragma unroll
    for (int r_ = 0; r_ < 3; r_++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // (G K^T)_rc = sum_q G_rq K_cq;  (K^T G)_rc = sum_q K_qr G_qc
            const double gkt = G[3 * r_] * K[3 * c] + G[3 * r_ + 1] * K[3 * c + 1] + G[3 * r_ + 2] * K[3 * c + 2];
            const double ktg = K[r_] * G[c] + K[3 + r_] * G[3 + c] + K[6 + r_] * G[6 + c];
            gK[3 * r_ + c] = sn * G[3 * r_ + c] + cc * (gkt + ktg);
        }
    const double gkx = gK[7] - gK[5], gky = gK[2] - gK[6], gkz = gK[3] - gK[1];
    const double g_a = g_s * cs + g_c * sn - (gkx * rx + gky * ry + gkz * rz) / (a * a);
    g_r[0] = (float)(gkx / a + g_a * ex / a);
    g_r[1] = (float)(gky / a + g_a * ey / a);
    g_r[2] = (float)(gkz / a + g_a * ez / a);
}

// this workgroup's share of J_regressor v_shaped for its nv vertices from v0, per shape set: partials [workgroup][J][S][3]
template <int S, int BLOCK>
__device__ __forceinline__ void smpl_regressor_shares(const float* jreg, int V, int J, int v0, int nv, const double (*s_vs)[SMPL_VPB * 3],
                                                      double* __restrict__ partials)
{
    for (int o = threadIdx.x; o < J * 3 * S; o += BLOCK) {
        const int j = o / (3 * S), s = (o % (3 * S)) / 3, c = o % 3;
        const float* jr = jreg + (size_t)j * V + v0;
        double acc = 0.0;
        for (int i = 0; i < nv; i++) acc = fma((double)jr[i], s_vs[s][3 * i + c], acc);
        partials[(size_t)blockIdx.x * J * 3 * S + o] = acc;
    }
}

// rows [0, nrows) from vertex v0 of posedirs f: one wave per 4 rows, lanes over the feature, a fixed butterfly; store(row, sum)
template <int BLOCK, typename Store>
__device__ __forceinline__ void smpl_pose_blend_rows(const float* pd, const float* s_f, int F, int v0, int nrows, Store store)
{
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int r0 = wave * 4; r0 < nrows; r0 += 4 * (BLOCK / 64)) {
        const float* p0 = pd + ((size_t)v0 * 3 + r0) * F;
        const float* p1 = pd + ((size_t)v0 * 3 + min(r0 + 1, nrows - 1)) * F;       // (rows past the range: read again, not written)
        const float* p2 = pd + ((size_t)v0 * 3 + min(r0 + 2, nrows - 1)) * F;
        const float* p3 = pd + ((size_t)v0 * 3 + min(r0 + 3, nrows - 1)) * F;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int k = lane; k < F; k += 64) {
            const double f = (double)s_f[k];
            a0 = fma((double)p0[k], f, a0); a1 = fma((double)p1[k], f, a1);
            a2 = fma((double)p2[k], f, a2); a3 = fma((double)p3[k], f, a3);
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
        if (lane < 4 && r0 + lane < nrows) store(r0 + lane, lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3);
    }
}

// the joints from the shares of nparts workgroups: every output's shares are cut into nslice = BLOCK / (3 S J) runs of workgroups,
// each summed in order, then the runs in order -- a function of V and J only.  Ends with the workgroup in step.
template <int S, int BLOCK>
__device__ __forceinline__ void smpl_fold_shares(int J, int nparts, const double* __restrict__ partials, double* s_slice,
                                                 double (*s_jt)[SMPL_MAX_J * 3])
{
    const int t = threadIdx.x, nout = J * 3 * S;
    const int nslice = BLOCK / nout;
    const int per = (nparts + nslice - 1) / nslice;
    if (t < nout * nslice) {
        const int o = t % nout, sl = t / nout;
        const int b1 = min(nparts, (sl + 1) * per);
        double acc = 0.0;
        for (int b = sl * per; b < b1; b++) acc += partials[(size_t)b * nout + o];
        s_slice[t] = acc;
    }
    __syncthreads();
    if (t < nout) {
        double acc = 0.0;
        for (int sl = 0; sl < nslice; sl++) acc += s_slice[sl * nout + t];
        s_jt[(t % (3 * S)) / 3][3 * (t / (3 * S)) + t % 3] = acc;
    }
    __syncthreads();
}

// rel_0 = joint_0, rel_j = joint_j - joint_parent[j], per shape set.  Ends with the workgroup in step.
template <int S>
__device__ __forceinline__ void smpl_relative_joints(int J, const SmplParents& par, const double (*s_jt)[SMPL_MAX_J * 3],
                                                     double (*s_rel)[SMPL_MAX_J * 3])
{
    const int t = threadIdx.x;
    if (t < S * J * 3) {
        const int s = S == 1 ? 0 : t / (J * 3), e = S == 1 ? t : t % (J * 3), j = e / 3, c = e % 3;
        s_rel[s][e] = j == 0 ? s_jt[s][e] : s_jt[s][e] - s_jt[s][3 * par.p[j] + c];
    }
    __syncthreads();
}

// entry e of G_j = G_parent[j] [R_j | rel_j] (the root: [R_0 | rel_0]) of the chain Gs: per joint the rotation (9, row-major), then
// the translation (3).  One joint per step: parent[j] < j is all that is known of the tree.
__device__ __forceinline__ void smpl_chain_step(int j, int e, const SmplParents& par, const float* R, const double* rel, double* Gs)
{
    double* G = Gs + 12 * j;
    if (j == 0) {
        G[e] = e < 9 ? (double)R[e] : rel[e - 9];
    } else {
        const double* Gp = Gs + 12 * par.p[j];
        if (e < 9) {
            const int r = e / 3, c = e % 3;
            G[e] = Gp[3 * r] * (double)R[c] + Gp[3 * r + 1] * (double)R[3 + c] + Gp[3 * r + 2] * (double)R[6 + c];
        } else {
            const int r = e - 9;
            G[e] = Gp[3 * r] * rel[0] + Gp[3 * r + 1] * rel[1] + Gp[3 * r + 2] * rel[2] + Gp[9 + r];
        }
    }
}

// A_j[r][c] for r < 3: [G_j.R | G_j.t - G_j.R joint_j]
__device__ __forceinline__ double smpl_A_entry(const double* G, const double* jt, int r, int c)
{
    return c < 3 ? G[3 * r + c] : G[9 + r] - (G[3 * r] * jt[0] + G[3 * r + 1] * jt[1] + G[3 * r + 2] * jt[2]);
}

}  // namespace moss
