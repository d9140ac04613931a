// metrics.hip -- the evaluation metrics of MOSS's test / train reports, forward only, up to eight views per launch
// (include/moss_raster.h moss_eval_metrics).  Per view, exactly what train_ZJU.py:244-253 (training_report) computes:
//     image = clamp(render, 0, 1); gt = clamp(gt, 0, 1); image[bound_mask == 0] = fill      (fill: 0 on a black background, else 1)
//     l1   = mean |image - gt|                                             (utils/loss_utils.py:41-42, over all C*H*W elements)
//     psnr = mean over channels of 20 log10(1 / sqrt(mse_c))               (utils/image_utils.py:19-21: psnr of a (C,H,W) image viewed
//                                                                           as (C, H*W), then .mean() -- NOT the psnr of the total mse)
//     ssim = mean SSIM map, 11x11 window, sigma 1.5, zero padding          (utils/loss_utils.py:47-87, the full frame)
// and adds the three float32 values, view after view, into float64 running sums (`l1_test += l1_loss(...).mean().double()`).
//
// Two launches, nothing synchronous, no float atomics:
//   tiles: per 32 x 32 tile, channel and view, the clamped and filled x and y tiles (+5 px halo) go to LDS once and the four windowed
//          moments E[x], E[y], E[x^2 + y^2], E[xy] are formed separably -- the scheme and the XCD tile order of loss.hip pass 1 -- then
//          the SSIM map, |x - y| and (x - y)^2 are summed over the tile into three floats of the workspace; the clamped and filled
//          render is written to `out_image` on request (what the caller's LPIPS reads);
//   fold:  one workgroup, one wave per view, folds each view's tile sums in a fixed order in float64, forms the three float32 metrics
//          and adds them into the state block in view order.  Bitwise reproducible; every address the second kernel reads was written
//          by the first.
// Traffic per view and channel: 2 x 4 B read per pixel (+ the halo re-reads, mostly from L2) + 1 B of the mask, + 4 B written with out_image.
#include "common.h"
#include "ssim_tiles.h"

namespace moss {

namespace {

constexpr int MAX_VIEWS = 8;
constexpr int MAX_CH = 4;


struct Views {
    const float* image[MAX_VIEWS];
    const float* gt[MAX_VIEWS];
    const unsigned char* bound[MAX_VIEWS];
    float* out[MAX_VIEWS];
};

// torch.clamp(v, 0, 1): NaN stays NaN
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__global__ void __launch_bounds__(256)
eval_tiles_kernel(Views V, int C, int H, int W, int gx, int gy, float fill, Win win, float* __restrict__ partials /* [views][C][gy][gx][3] */)
{
    __shared__ float s_x[LP][LP + 1];
    __shared__ float s_y[LP][LP + 1];
    __shared__ float s_h[4][LP][LT + 1];               // (36.7 KB of LDS in all: four workgroups per CU)
    __shared__ float s_red[3][4];

    // XCD-aware order (ssim_tiles.h xcd_order) over the (view, channel, row, column) sequence: the tiles that re-read each other's halo
    // share an L2
    const int t = xcd_order((int)blockIdx.x, (int)gridDim.x);
    const int per_view = C * gy * gx;
    const int view = t / per_view, rem = t % per_view;
    const int c = rem / (gy * gx), by = (rem / gx) % gy, bx = rem % gx;

    // this view's pointers (static indices: a run-time index into the argument struct would be copied to private memory first)
    const float* xi = nullptr; const float* yi = nullptr; const unsigned char* bd = nullptr; float* out = nullptr;
#pragma unroll
    for (int v = 0; v < MAX_VIEWS; v++)
        if (v == view) { xi = V.image[v]; yi = V.gt[v]; bd = V.bound[v]; out = V.out[v]; }

    const size_t plane = (size_t)H * W;
    const float* xc = xi + (size_t)c * plane;
    const float* yc = yi + (size_t)c * plane;
    const int x0 = bx * LT, y0 = by * LT;
    const int tid = threadIdx.x;
    {
        // tile + halo: all loads first (clamped addresses, in flight together), then clamp / fill / zero padding into LDS
        constexpr int NLD = (LP * LP + 255) / 256;
        float vx[NLD], vy[NLD];
        unsigned char vb[NLD];
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / LP, q = i % LP;
            const size_t o = (size_t)min(max(y0 + r - HALO, 0), H - 1) * W + min(max(x0 + q - HALO, 0), W - 1);
            vx[k] = xc[o]; vy[k] = yc[o];
            vb[k] = bd != nullptr ? bd[o] : (unsigned char)1;
        }
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / LP, q = i % LP;
            const int gx_ = x0 + q - HALO, gy_ = y0 + r - HALO;
            const bool in = gx_ >= 0 && gx_ < W && gy_ >= 0 && gy_ < H;
            if (i < LP * LP) {
                const float a = vb[k] ? clamp01(vx[k]) : fill;          // the fill goes onto the render only, after its clamp
                s_x[r][q] = in ? a : 0.0f;
                s_y[r][q] = in ? clamp01(vy[k]) : 0.0f;
            }
        }
    }
    __syncthreads();
    if (tid < (LT / SEG) * LP) {                        // horizontal 11-tap of the four moments (ssim_tiles.h ssim_filter_h)
        const int r = tid % LP, q0 = (tid / LP) * SEG;
        v2f a01[SEG], a23[SEG];
#pragma unroll
        for (int j = 0; j < SEG; j++) { a01[j] = v2f{0.f, 0.f}; a23[j] = v2f{0.f, 0.f}; }
#pragma unroll
        for (int i = 0; i < SEG + 10; i++) {
            const float a = s_x[r][q0 + i], b = s_y[r][q0 + i];
            const v2f ab = v2f{a, b}, sq = ab * ab;
            const v2f sx = v2f{sq.x + sq.y, a * b};                                // (x^2 + y^2, x y)
#pragma unroll
            for (int j = 0; j < SEG; j++) {
                if (i - j >= 0 && i - j <= 10) {
                    const float w = win.g[i - j];
                    const v2f w2 = v2f{w, w};
                    a01[j] = __builtin_elementwise_fma(w2, ab, a01[j]); a23[j] = __builtin_elementwise_fma(w2, sx, a23[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SEG; j++) {
            s_h[0][r][q0 + j] = a01[j].x; s_h[1][r][q0 + j] = a01[j].y; s_h[2][r][q0 + j] = a23[j].x; s_h[3][r][q0 + j] = a23[j].y;
        }
    }
    __syncthreads();
    const int lx = tid % LT, ly0 = (tid / LT) * VR;     // vertical: column lx, rows ly0 .. ly0 + VR - 1
    v2f m01[VR], m23[VR];
#pragma unroll
    for (int j = 0; j < VR; j++) { m01[j] = v2f{0.f, 0.f}; m23[j] = v2f{0.f, 0.f}; }
#pragma unroll
    for (int i = 0; i < VR + 10; i++) {
        const v2f v01 = v2f{s_h[0][ly0 + i][lx], s_h[1][ly0 + i][lx]}, v23 = v2f{s_h[2][ly0 + i][lx], s_h[3][ly0 + i][lx]};
#pragma unroll
        for (int j = 0; j < VR; j++) {
            if (i - j >= 0 && i - j <= 10) {
                const float w = win.g[i - j];
                const v2f w2 = v2f{w, w};
                m01[j] = __builtin_elementwise_fma(w2, v01, m01[j]); m23[j] = __builtin_elementwise_fma(w2, v23, m23[j]);
            }
        }
    }
    float ssim_v = 0.f, l1_v = 0.f, sq_v = 0.f;
    const int px = x0 + lx;
#pragma unroll
    for (int j = 0; j < VR; j++) {
        const int ly = ly0 + j, py = y0 + ly;
        if (px < W && py < H) {
            const float mu1 = m01[j].x, mu2 = m01[j].y, ess = m23[j].x /* E[x^2 + y^2] */, exy = m23[j].y;
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float sigma12 = exy - mu1_mu2;
            // sigma1^2 + sigma2^2 = E[x^2 + y^2] - mu1^2 - mu2^2 (as ssim_tiles.h ssim_point); utils/loss_utils.py:84 with a true division (forward only:
            // no derivatives share the reciprocals here)
            const float S = ((2.f * mu1_mu2 + C1) * (2.f * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * ((ess - mu1_sq - mu2_sq) + C2));
            ssim_v += S;
            const float x = s_x[ly + HALO][lx + HALO], d = x - s_y[ly + HALO][lx + HALO];
            l1_v += fabsf(d);
            sq_v += d * d;
            if (out != nullptr) out[(size_t)c * plane + (size_t)py * W + px] = x;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { ssim_v += __shfl_xor(ssim_v, d); l1_v += __shfl_xor(l1_v, d); sq_v += __shfl_xor(sq_v, d); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = l1_v; s_red[1][tid >> 6] = sq_v; s_red[2][tid >> 6] = ssim_v; }
    __syncthreads();
    if (tid == 0) {
        float* p = partials + (size_t)t * 3;             // (t: the logical tile id -- view, channel, row, column)
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = block_sum3(s_red, k);
    }
}

// One workgroup of MAX_VIEWS waves: wave b folds view b's tile sums (lane l takes tiles l, l + 64, ... in float64; then a fixed
// butterfly), forms the view's three metrics; thread 0 adds them into the state in view order.
__global__ void __launch_bounds__(64 * MAX_VIEWS)
eval_fold_kernel(int B, int C, int H, int W, int tiles /* gx * gy */, const float* __restrict__ partials, double* __restrict__ state,
                 float* __restrict__ per_view, int per_view_capacity)
{
    __shared__ float s_m[MAX_VIEWS][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave < B) {
        const float* p = partials + (size_t)wave * C * tiles * 3;
        double l1 = 0.0, ss = 0.0, sq[MAX_CH] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < C; c++) {
            double s = 0.0;
            for (int i = lane; i < tiles; i += 64) {
                const float* q = p + ((size_t)c * tiles + i) * 3;
                l1 += (double)q[0]; s += (double)q[1]; ss += (double)q[2];
            }
#pragma unroll
            for (int k = 0; k < MAX_CH; k++) if (k == c) sq[k] = s;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            l1 += __shfl_xor(l1, d); ss += __shfl_xor(ss, d);
#pragma unroll
            for (int k = 0; k < MAX_CH; k++) sq[k] += __shfl_xor(sq[k], d);
        }
        if (lane == 0) {
            const double n_pix = (double)H * (double)W, n = (double)C * n_pix;
            double psnr = 0.0;
#pragma unroll
            for (int k = 0; k < MAX_CH; k++)
                if (k < C) psnr += 20.0 * log10(1.0 / sqrt(sq[k] / n_pix));      // mse 0 -> +inf, as torch
            s_m[wave][0] = (float)(l1 / n);
            s_m[wave][1] = (float)(psnr / (double)C);
            s_m[wave][2] = (float)(ss / n);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // state: double sums [0] l1, [1] psnr, [2] ssim; [3] the number of views added (int64); [4..7] untouched (the caller's)
        long long n0 = reinterpret_cast<const long long*>(state)[3];
        double a = state[0], b = state[1], c = state[2];
        for (int v = 0; v < B; v++) {
            a += (double)s_m[v][0]; b += (double)s_m[v][1]; c += (double)s_m[v][2];
            if (per_view != nullptr && n0 + v >= 0 && n0 + v < (long long)per_view_capacity) {
                float* o = per_view + (size_t)(n0 + v) * 3;
                o[0] = s_m[v][0]; o[1] = s_m[v][1]; o[2] = s_m[v][2];
            }
        }
        state[0] = a; state[1] = b; state[2] = c;
        reinterpret_cast<long long*>(state)[3] = n0 + B;
    }
}

}  // anonymous namespace
}  // namespace moss

using namespace moss;

extern "C" size_t moss_metrics_workspace_bytes(int B, int C, int H, int W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    const size_t gx = (W + LT - 1) / LT, gy = (H + LT - 1) / LT;
    return align_up((size_t)B * C * gx * gy * 3 * 4);
}

extern "C" size_t moss_metrics_state_bytes(void) { return MOSS_METRICS_STATE_BYTES; }

extern "C" int moss_eval_metrics(const moss_eval_metrics_args* a, void* stream)
{
    if (!a || a->num_views < 1 || a->num_views > MAX_VIEWS) return MOSS_ERR_INVALID_ARG;
    const int B = a->num_views, C = a->C, H = a->H, W = a->W;
    if (C < 1 || C > MAX_CH || H <= 0 || W <= 0 || !a->state || !a->workspace) return MOSS_ERR_INVALID_ARG;
    if (a->per_view_capacity < 0 || (a->per_view_capacity > 0 && !a->per_view)) return MOSS_ERR_INVALID_ARG;
    if (a->workspace_bytes < moss_metrics_workspace_bytes(B, C, H, W)) return MOSS_ERR_INVALID_ARG;
    const int gx = (W + LT - 1) / LT, gy = (H + LT - 1) / LT;
    if ((long long)B * C * gx * gy > 0x7fffffffLL) return MOSS_ERR_INVALID_ARG;
    Views V;
    for (int v = 0; v < MAX_VIEWS; v++) {
        const bool on = v < B;
        V.image[v] = on ? a->image[v] : nullptr; V.gt[v] = on ? a->gt[v] : nullptr;
        V.bound[v] = on ? a->bound[v] : nullptr; V.out[v] = on ? a->out_image[v] : nullptr;
        if (on && (!V.image[v] || !V.gt[v])) return MOSS_ERR_INVALID_ARG;
    }
    static const Win win = make_window();
    hipStream_t s = (hipStream_t)stream;
    float* partials = reinterpret_cast<float*>(a->workspace);
    hipLaunchKernelGGL(eval_tiles_kernel, dim3(B * C * gx * gy), dim3(256), 0, s, V, C, H, W, gx, gy, a->fill, win, partials);
    hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(64 * MAX_VIEWS), 0, s, B, C, H, W, gx * gy, (const float*)partials,
                       (double*)a->state, a->per_view, a->per_view_capacity);
    return hipGetLastError() == hipSuccess ? 0 : MOSS_ERR_HIP;
}
