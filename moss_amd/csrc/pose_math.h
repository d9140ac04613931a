// pose_math.h -- the per-matrix arithmetic of pose_head.hip: MOSS's Rodrigues formula and its adjoint, a 3x3 SVD by one-sided Jacobi
// rotations, and the integrand of the matrix-Fisher normalising constant.  Host + device, so that the same code can be checked on a CPU.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define POSE_HD __host__ __device__ __forceinline__
#else
#define POSE_HD inline
#endif

namespace moss {
namespace pose {

constexpr int QUAD_POINTS = 512;

// RodriguesModule (nets/mlp_delta_body_pose.py:258-284): th = sqrt(1e-5 + |r|^2), n = r / th (NOT a unit vector),
// R = n n^T (1 - cos th) + cos th I + sin th [n]x, row-major.
POSE_HD void rodrigues(const float r[3], float R[9])
{
    const float th = sqrtf(1e-5f + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
    const float x = r[0] / th, y = r[1] / th, z = r[2] / th;
    const float c = cosf(th), s = sinf(th), k = 1.0f - c;
    R[0] = x * x + (1.0f - x * x) * c; R[1] = x * y * k - z * s;          R[2] = x * z * k + y * s;
    R[3] = x * y * k + z * s;          R[4] = y * y + (1.0f - y * y) * c; R[5] = y * z * k - x * s;
    R[6] = x * z * k - y * s;          R[7] = y * z * k + x * s;          R[8] = z * z + (1.0f - z * z) * c;
}

// dr = (dR/dr)^T G for the formula above.  With R_ab = n_a n_b (1 - c) + d_ab c + s K_ab(n):
//   dL/dn = (1 - c)(G + G^T) n + s kv,  kv = (G21 - G12, G02 - G20, G10 - G01);   dL/dc = tr G - n^T G n;   dL/ds = n . kv
//   n = r / th and dth/dr = n:   dr = dL/dn / th + n (c dL/ds - s dL/dc - (dL/dn . n) / th)
POSE_HD void rodrigues_adjoint(const float r[3], const float G[9], float dr[3])
{
    const float th = sqrtf(1e-5f + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
    const float n[3] = {r[0] / th, r[1] / th, r[2] / th};
    const float c = cosf(th), s = sinf(th), k = 1.0f - c;
    const float kv[3] = {G[7] - G[5], G[2] - G[6], G[3] - G[1]};
    float dn[3], nGn = 0.0f;
    for (int a = 0; a < 3; a++) {
        float sym = 0.0f, row = 0.0f;
        for (int b = 0; b < 3; b++) { sym += (G[3 * a + b] + G[3 * b + a]) * n[b]; row += G[3 * a + b] * n[b]; }
        dn[a] = k * sym + s * kv[a];
        nGn += n[a] * row;
    }
    const float dc = (G[0] + G[4] + G[8]) - nGn;
    const float ds = n[0] * kv[0] + n[1] * kv[1] + n[2] * kv[2];
    const float dn_n = dn[0] * n[0] + dn[1] * n[1] + dn[2] * n[2];
    const float along = c * ds - s * dc - dn_n / th;
    for (int a = 0; a < 3; a++) dr[a] = dn[a] / th + n[a] * along;
}

struct Svd3 {
    float U[9], V[9];   // row-major; A = U diag(s) V^T
    float s[3];         // descending, >= 0
    float det;          // det(U V^T) = +1 or -1: the proper singular values are (s0, s1, s2 * det)
};

// One-sided Jacobi (Hestenes): plane rotations from the right make the columns of A V orthogonal; their norms are the singular
// values -- accurate to a few ulp of the largest also when singular values coincide (a rotation-like A converges in one sweep).
POSE_HD void svd3(const float A[9], Svd3& o)
{
    float a[3][3], v[3][3];      // a[i] = column i of A V, v[i] = column i of V
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { a[i][j] = A[3 * j + i]; v[i][j] = i == j ? 1.0f : 0.0f; }
    for (int sweep = 0; sweep < 12; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int pair = 0; pair < 3; pair++) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const float alpha = a[p][0] * a[p][0] + a[p][1] * a[p][1] + a[p][2] * a[p][2];
            const float beta = a[q][0] * a[q][0] + a[q][1] * a[q][1] + a[q][2] * a[q][2];
            const float gamma = a[p][0] * a[q][0] + a[p][1] * a[q][1] + a[p][2] * a[q][2];
            if (fabsf(gamma) > 3e-8f * sqrtf(alpha * beta)) {
                rotated = true;
                const float zeta = (beta - alpha) / (2.0f * gamma);
                const float t = (zeta >= 0.0f ? 1.0f : -1.0f) / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
                const float c = 1.0f / sqrtf(1.0f + t * t), s = c * t;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float ap = a[p][j], aq = a[q][j], vp = v[p][j], vq = v[q][j];
                    a[p][j] = c * ap - s * aq; a[q][j] = s * ap + c * aq;
                    v[p][j] = c * vp - s * vq; v[q][j] = s * vp + c * vq;
                }
            }
        }
        if (!rotated) break;
    }
    float sg[3];
#pragma unroll
    for (int i = 0; i < 3; i++) sg[i] = sqrtf(a[i][0] * a[i][0] + a[i][1] * a[i][1] + a[i][2] * a[i][2]);
    // descending order (swapping a column of A V with the same column of V keeps det(U) det(V))
#pragma unroll
    for (int pair = 0; pair < 3; pair++) {
        const int p = pair == 1 ? 1 : 0, q = pair == 1 ? 2 : 1;        // (0,1), (1,2), (0,1)
        if (sg[p] < sg[q]) {
            float t = sg[p]; sg[p] = sg[q]; sg[q] = t;
#pragma unroll
            for (int j = 0; j < 3; j++) { t = a[p][j]; a[p][j] = a[q][j]; a[q][j] = t; t = v[p][j]; v[p][j] = v[q][j]; v[q][j] = t; }
        }
    }
    float u[3][3];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) u[i][j] = a[i][j] / sg[i];
    const float cx[3] = {u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2], u[0][0] * u[1][1] - u[0][1] * u[1][0]};
    if (sg[2] > 1e-4f * sg[0]) {
#pragma unroll
        for (int j = 0; j < 3; j++) u[2][j] = a[2][j] / sg[2];
    } else {
        // a (nearly) vanishing third singular value: its column has no direction of its own; complete the basis, on the column's side
        const float side = (cx[0] * a[2][0] + cx[1] * a[2][1] + cx[2] * a[2][2]) < 0.0f ? -1.0f : 1.0f;
#pragma unroll
        for (int j = 0; j < 3; j++) u[2][j] = side * cx[j];
    }
    const float det_u = cx[0] * u[2][0] + cx[1] * u[2][1] + cx[2] * u[2][2];
    const float det_v = (v[0][1] * v[1][2] - v[0][2] * v[1][1]) * v[2][0] + (v[0][2] * v[1][0] - v[0][0] * v[1][2]) * v[2][1]
                      + (v[0][0] * v[1][1] - v[0][1] * v[1][0]) * v[2][2];
    o.det = det_u * det_v < 0.0f ? -1.0f : 1.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        o.s[i] = sg[i];
#pragma unroll
        for (int j = 0; j < 3; j++) { o.U[3 * j + i] = u[i][j]; o.V[3 * j + i] = v[i][j]; }
    }
}

// M = U diag(d) V^T, row-major
POSE_HD void u_diag_vt(const float U[9], const float V[9], const float d[3], float M[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            M[3 * i + j] = U[3 * i] * d[0] * V[3 * j] + U[3 * i + 1] * d[1] * V[3 * j + 1] + U[3 * i + 2] * d[2] * V[3 * j + 2];
}

// exp(-|x|) I0(x): the polynomial pair of utils/loss_utils.py:98-133 (Abramowitz & Stegun 9.8.1 / 9.8.2), split at |x| <= 3.75.
// x = 0 takes the first branch: exactly 1.
POSE_HD float bessel0_scaled(float x)
{
    const float a = fabsf(x);
    if (a <= 3.75f) {
        float t = a / 3.75f;
        t *= t;
        float z = 0.45813e-2f;
        z = z * t + 0.360768e-1f; z = z * t + 0.2659732f; z = z * t + 1.2067492f; z = z * t + 3.0899424f; z = z * t + 3.5156229f;
        z = z * t + 1.0f;
        return z / expf(a);
    }
    const float t = 3.75f / a;
    float z = 0.392377e-2f;
    z = z * t + -0.1647633e-1f; z = z * t + 0.2635537e-1f; z = z * t + -0.2057706e-1f; z = z * t + 0.916281e-2f;
    z = z * t + -0.157565e-2f; z = z * t + 0.225319e-2f; z = z * t + 0.1328592e-1f; z = z * t + 0.39894228f;
    return z / sqrtf(a);
}

// point i of the 512-point trapezoid on [-1, 1] and its weight
POSE_HD float quad_u(int i) { return (float)i * (2.0f / (QUAD_POINTS - 1)) + -1.0f; }
POSE_HD float quad_w(int i) { return (i == 0 || i == QUAD_POINTS - 1) ? 0.5f : 1.0f; }

// I0~((si - sj)(1 - u)/2) I0~((si + sj)(1 + u)/2) exp((sj + sk)(u - 1)): the integrand of c~(S) with (si, sj, sk) = (S2, S3, S1)
// (utils/loss_utils.py:161-184); times u, over a cyclic shift, the integrand of dc~/dS_k + c~ (:187-219)
POSE_HD float mf_integrand(float si, float sj, float sk, float u)
{
    return bessel0_scaled((si - sj) * 0.5f * (1.0f - u)) * bessel0_scaled((si + sj) * 0.5f * (1.0f + u)) * expf((sj + sk) * (u - 1.0f));
}

// the scaling of a trapezoid sum: 0.5 * (sum * (1 - -1) / 511)
POSE_HD float quad_scale(float sum) { return 0.5f * (sum * 2.0f / (QUAD_POINTS - 1)); }

// the (si, sj, sk) of derivative k: the cyclic shift that puts S_k first, the other two as (max, min)
POSE_HD void shift_args(const float S[3], int k, float& si, float& sj, float& sk)
{
    const float a = S[(k + 1) % 3], b = S[(k + 2) % 3];
    si = fmaxf(a, b); sj = fminf(a, b); sk = S[k];
}

}  // namespace pose
}  // namespace moss
