// keypoints.hip -- a keypoint loss on posed vertices, value and vertex gradient in one call (include/moss_raster.h moss_keypoint_loss; the
// formulas are restated there): keypoints as a dense regressor over the vertices, their projection into C cameras with
// moss_bound_mask's convention (frame_bounds.hip), a Geman-McClure robustifier on the 2D and the 3D residuals.
//
// 3 launches:
//   keypoints  one workgroup per keypoint: X_k = sum_v regressor[k, v] world_vertex[v]; threads stride the vertices, then a fixed
//              butterfly and the waves in order.  X stays in float64 in the workspace.
//   residuals  one workgroup per camera and one more for the 3D part, one thread per keypoint: the entry's value and its gradient to
//              X_k; the workgroup's values are summed in keypoint order; flags[c] is written.
//   scatter    a grid over ranges of KP_BLOCK vertices: every workgroup folds g_X over the cameras in camera order (workgroup 0 also the
//              loss), then g_world_vertex[v] = sum_k regressor[k, v] g_X[k] in keypoint order.
// Every sum is formed in float64 in a fixed order, nothing is atomic, every output element is written: bitwise reproducible.
// Nothing is allocated, nothing synchronises, nothing is cleared with a memset.  Every loop's trip count is fixed by V, Kp and C.
#include "common.h"
#include "wave.h"

namespace moss {

namespace {

constexpr int KP_BLOCK = 256;
constexpr int KP_MAX = MOSS_KEYPOINTS_MAX;

struct KpIn {
    int Kp, C;
    const float* K;
    const float* RT;
    const float* uv;
    const float* conf;
    const float* xyz;
    const float* conf3;
    float sigma, sigma3;
};

// X[k] (float64) and keypoints[k] of keypoint blockIdx.x
__global__ void __launch_bounds__(KP_BLOCK)
keypoint_regress_kernel(int V, const float* __restrict__ world_vertex, const float* __restrict__ regressor, double* __restrict__ X,
                        float* __restrict__ keypoints)
{
    __shared__ double s_w[KP_BLOCK / 64][3];
    const int t = threadIdx.x, k = blockIdx.x;
    const float* row = regressor + (size_t)k * V;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 4
    for (int v = t; v < V; v += KP_BLOCK) {
        const double w = (double)row[v];
        const float* p = world_vertex + (size_t)v * 3;
        a0 = fma(w, (double)p[0], a0); a1 = fma(w, (double)p[1], a1); a2 = fma(w, (double)p[2], a2);
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (t % 64 == 0) { s_w[t / 64][0] = a0; s_w[t / 64][1] = a1; s_w[t / 64][2] = a2; }
    __syncthreads();
    if (t < 3) {
        double acc = s_w[0][t];
        for (int wv = 1; wv < KP_BLOCK / 64; wv++) acc += s_w[wv][t];
        X[3 * k + t] = acc;
        if (keypoints) keypoints[3 * k + t] = (float)acc;
    }
}

// rho_s(r2) = s^2 r2 / (s^2 + r2) and its derivative (s^2 / (s^2 + r2))^2; r2 and 1 for s <= 0
__device__ __forceinline__ void kp_rho(float sigma, double r2, double& rho, double& drho)
{
    if (sigma > 0.0f) {
        const double s2 = (double)sigma * (double)sigma;
        const double q = s2 / (s2 + r2);
        rho = q * r2;
        drho = q * q;
    } else {
        rho = r2;
        drho = 1.0;
    }
}

// camera blockIdx.x < C, or the 3D part (blockIdx.x == C): gx[part][k][3] = conf d rho / d X_k, lossp[part] = sum_k conf rho
__global__ void __launch_bounds__(KP_MAX)
keypoint_residual_kernel(KpIn a, const double* __restrict__ X, double* __restrict__ gx, double* __restrict__ lossp,
                         int32_t* __restrict__ flags)
{
    __shared__ double s_val[KP_MAX];
    const int k = threadIdx.x, c = blockIdx.x;
    double val = 0.0, g[3] = {0.0, 0.0, 0.0};
    int behind = 0;
    if (k < a.Kp) {
        const double x0 = X[3 * k], x1 = X[3 * k + 1], x2 = X[3 * k + 2];
        if (c < a.C) {
            const float* RT = a.RT + (size_t)c * 12;
            const float* K = a.K + (size_t)c * 9;
            double cam[3], uvw[3];
#pragma unroll
            for (int r = 0; r < 3; r++)
                cam[r] = (double)RT[4 * r] * x0 + (double)RT[4 * r + 1] * x1 + (double)RT[4 * r + 2] * x2 + (double)RT[4 * r + 3];
#pragma unroll
            for (int r = 0; r < 3; r++) uvw[r] = (double)K[3 * r] * cam[0] + (double)K[3 * r + 1] * cam[1] + (double)K[3 * r + 2] * cam[2];
            if (uvw[2] <= 0.0) {
                behind = 1;                                    // (moss_bound_mask's rule: the entry adds nothing)
            } else {
                const size_t e = (size_t)c * a.Kp + k;
                const double z = uvw[2], u = uvw[0] / z, v = uvw[1] / z;
                const double du = u - (double)a.uv[2 * e], dv = v - (double)a.uv[2 * e + 1];
                const double w = (double)a.conf[e];
                double rho, drho;
                kp_rho(a.sigma, du * du + dv * dv, rho, drho);
                val = w * rho;
                const double gu = 2.0 * w * drho * du, gv = 2.0 * w * drho * dv;
                const double q[3] = {gu / z, gv / z, -(gu * u + gv * v) / z};           // the gradient of uvw
                double gc[3];
#pragma unroll
                for (int i = 0; i < 3; i++) gc[i] = (double)K[i] * q[0] + (double)K[3 + i] * q[1] + (double)K[6 + i] * q[2];      // K^T
#pragma unroll
                for (int i = 0; i < 3; i++) g[i] = (double)RT[i] * gc[0] + (double)RT[4 + i] * gc[1] + (double)RT[8 + i] * gc[2];  // RT[:, :3]^T
            }
        } else {
            const double d0 = x0 - (double)a.xyz[3 * k], d1 = x1 - (double)a.xyz[3 * k + 1], d2 = x2 - (double)a.xyz[3 * k + 2];
            const double w = (double)a.conf3[k];
            double rho, drho;
            kp_rho(a.sigma3, d0 * d0 + d1 * d1 + d2 * d2, rho, drho);
            val = w * rho;
            g[0] = 2.0 * w * drho * d0; g[1] = 2.0 * w * drho * d1; g[2] = 2.0 * w * drho * d2;
        }
        double* out = gx + ((size_t)c * a.Kp + k) * 3;
        out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
    }
    s_val[k] = val;
    const int any = __syncthreads_or(behind);
    if (k == 0) {
        double acc = 0.0;
        for (int i = 0; i < a.Kp; i++) acc += s_val[i];
        lossp[c] = acc;
        if (c < a.C) flags[c] = any ? 1 : 0;
    }
}

// g_X[k] = s2 sum_c gx[c][k] + s3 gx[C][k] (the cameras in order), then the vertices of this workgroup; workgroup 0: the loss
__global__ void __launch_bounds__(KP_BLOCK)
keypoint_scatter_kernel(int V, int Kp, int C, int has3d, double s2, double s3, const float* __restrict__ regressor,
                        const double* __restrict__ gx, const double* __restrict__ lossp, float* __restrict__ g_world_vertex,
                        float* __restrict__ loss)
{
    __shared__ double s_gX[KP_MAX * 3];
    const int t = threadIdx.x;
    const int n = Kp * 3;
    for (int o = t; o < n; o += KP_BLOCK) {
        double acc = 0.0;
        for (int c = 0; c < C; c++) acc += gx[(size_t)c * n + o];
        acc *= s2;
        if (has3d) acc = fma(s3, gx[(size_t)C * n + o], acc);
        s_gX[o] = acc;
    }
    if (blockIdx.x == 0 && t == 0) {
        double acc = 0.0;
        for (int c = 0; c < C; c++) acc += lossp[c];
        acc *= s2;
        if (has3d) acc = fma(s3, lossp[C], acc);
        loss[0] = (float)acc;
    }
    __syncthreads();
    const int v = blockIdx.x * KP_BLOCK + t;
    if (v >= V) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = 0; k < Kp; k++) {
        const double w = (double)regressor[(size_t)k * V + v];
        a0 = fma(w, s_gX[3 * k], a0); a1 = fma(w, s_gX[3 * k + 1], a1); a2 = fma(w, s_gX[3 * k + 2], a2);
    }
    float* out = g_world_vertex + (size_t)v * 3;
    out[0] = (float)a0; out[1] = (float)a1; out[2] = (float)a2;
}

// X, then per part (C cameras and the 3D part) the gradients and the value
size_t kp_bytes(int C, int Kp)
{
    return align_up((size_t)Kp * 3 * sizeof(double)) + align_up(((size_t)C + 1) * Kp * 3 * sizeof(double))
         + align_up(((size_t)C + 1) * sizeof(double));
}

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_keypoint_loss_workspace_bytes(int C, int Kp)
{
    if (C < 0 || C > 65535 || Kp < 1 || Kp > KP_MAX) return 0;
    return kp_bytes(C, Kp);
}

extern "C" int moss_keypoint_loss(const moss_keypoint_loss_args* a, void* stream)
{
    const char* who = "moss_keypoint_loss";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (a->Kp < 1 || a->Kp > KP_MAX) return invalid_arg(who, "Kp must be 1..128");
    if (a->C < 0 || a->C > 65535) return invalid_arg(who, "C must be 0..65535");
    const bool has3d = a->xyz != nullptr;
    if (a->C == 0 && !has3d) return invalid_arg(who, "neither the 2D part (C >= 1) nor the 3D part (xyz) is present");
    if (!a->world_vertex || !a->regressor) return invalid_arg(who, "null input (world_vertex, regressor)");
    if (a->C > 0 && (!a->K || !a->RT || !a->uv || !a->conf)) return invalid_arg(who, "C >= 1 needs K, RT, uv and conf");
    if (has3d && !a->conf3) return invalid_arg(who, "xyz needs conf3");
    if (!a->loss || !a->g_world_vertex || (a->C > 0 && !a->flags)) return invalid_arg(who, "null output (loss, g_world_vertex, flags)");
    if (!a->workspace || a->workspace_bytes < kp_bytes(a->C, a->Kp))
        return invalid_arg(who, "needs moss_keypoint_loss_workspace_bytes(C, Kp) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    char* p = a->workspace;
    double* X = carve<double>(p, (size_t)a->Kp * 3);
    double* gx = carve<double>(p, ((size_t)a->C + 1) * a->Kp * 3);
    double* lossp = carve<double>(p, (size_t)a->C + 1);
    const KpIn in{a->Kp, a->C, a->K, a->RT, a->uv, a->conf, a->xyz, a->conf3, a->sigma, a->sigma3};
    const double s2 = a->C > 0 ? (double)a->weight2d / ((double)a->C * (double)a->Kp) : 0.0;
    const double s3 = has3d ? (double)a->weight3d / (double)a->Kp : 0.0;
    hipLaunchKernelGGL(keypoint_regress_kernel, dim3(a->Kp), dim3(KP_BLOCK), 0, s, a->V, a->world_vertex, a->regressor, X, a->keypoints);
    hipLaunchKernelGGL(keypoint_residual_kernel, dim3(a->C + (has3d ? 1 : 0)), dim3(KP_MAX), 0, s, in, (const double*)X, gx, lossp,
                       a->flags);
    hipLaunchKernelGGL(keypoint_scatter_kernel, dim3((a->V + KP_BLOCK - 1) / KP_BLOCK), dim3(KP_BLOCK), 0, s, a->V, a->Kp, a->C,
                       has3d ? 1 : 0, s2, s3, a->regressor, (const double*)gx, (const double*)lossp, a->g_world_vertex, a->loss);
    return launch_status(who);
}
