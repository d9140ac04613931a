// s3im.hip -- MOSS's S3IM loss term and its gradient (include/moss_raster.h moss_s3im_loss).
//
// MOSS calls s3im_fun(img_pred, img_gt) (utils/loss_utils.py:17-38, train_ZJU.py:123) with two (1,C,h,w) crops.  At batch 1 every
// randperm(1) is [0] and the reshape places each pixel R times side by side, so the term is deterministic:
//     s3im = 1 - SSIM(x~, y~),   x~[c][i][R j + r] = x[c][i][j]  (r = 0 .. R-1)
// with the SSIM of utils/loss_utils.py:47-87 (11x11 window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over C h R w).
// The widened images are never formed.  Two launches, as in loss.hip:
//   pass 1: per tile of TW source columns x 8 rows and channel: x, y (+ 5 rows, + 2 KH columns of halo) go to LDS; the four moments
//           (x, y, x^2 + y^2, xy) are filtered VERTICALLY first, over source rows (the widened image has the same rows); then, per
//           widened column R s + r, horizontally with phase weights h_r(k) = sum of the taps g[d + 5] whose column R s + r + d falls in
//           source column s + k (at most 2 KH + 1 source columns: KH = 1 for R >= 5).  SSIM and its derivatives w.r.t. E[x], E[x^2],
//           E[xy] are evaluated at every widened point in registers.  The backward's horizontal window, summed over the R replicas of
//           a source pixel, folds into source columns: W_fold(R k + r) = h_r(-k) (the window is symmetric), so pass 1 writes the three
//           derivative maps already folded -- 3 floats per SOURCE pixel-channel -- and its per-tile SSIM sums.
//   pass 2: the folded maps are filtered vertically (11 taps) and combined into dL/dx = -(F_mu + 2 x F_xx + y F_xy) / N; block 0 folds
//           the partial sums into {1 - ssim, ssim}.
// HBM traffic per source pixel-channel does not depend on R: (2 + 3) * 4 B in pass 1, (3 + 2 + 1) * 4 B in pass 2.  What R costs is
// R x the per-point SSIM arithmetic, in registers.  The crop (5 device ints, as moss_photometric_loss_roi reads them) and the tile
// orders are loss.hip's (ssim_tiles.h); tiles off the crop leave at once with zero gradients; sums in a fixed order, no atomics.
#include "common.h"
#include "ssim_tiles.h"

namespace moss {

namespace {

constexpr int S3_MAX_R = 16;
constexpr int P1_TH = 8;               // pass 1: rows per tile
constexpr int P1_NQ = 32;              // pass 1: source columns whose widened points a tile evaluates (TW + 2 KH: one per thread and row)
constexpr int P1_VR = 2;               // pass 1: rows per thread of the vertical filter
constexpr int P2_T = 32;               // pass 2: 32 x 32 tiles
constexpr int P2_VR = 4;               // pass 2: rows per thread
static_assert(P1_TH * P1_NQ == 256 && P2_T * (P2_T / P2_VR) == 256, "work split of a 256-thread workgroup");

// h[r][k + 5]: weight of source column s + k in the horizontal window of widened column R s + r (zero outside |k| <= KH)
struct PhaseTaps { float h[S3_MAX_R][11]; };

template <int KH> constexpr int p1_tw() { return P1_NQ - 2 * KH; }

__device__ __forceinline__ Crop s3im_crop(const int* __restrict__ rect, int W, int H)
{
    if (rect) return load_crop(rect, W, H, false);
    Crop r; r.x0 = 0; r.y0 = 0; r.x1 = W; r.y1 = H; r.n_pix = (float)W * (float)H; r.n_bound = r.n_pix;
    return r;
}

template <int KH>
__global__ void __launch_bounds__(256)
s3im_pass1_kernel(int C, int H, int W, int R, const float* __restrict__ img, const float* __restrict__ gt, Win win, PhaseTaps taps,
                  float* __restrict__ gmap /* [3][C][H][W] */, float* __restrict__ partials /* [blocks] */, const int* __restrict__ rect)
{
    constexpr int TW = p1_tw<KH>();
    constexpr int NV = TW + 4 * KH;    // columns of vertical moments (32 + 2 KH)
    constexpr int NL = P1_TH + 10;     // rows loaded
    constexpr int NK = 2 * KH + 1;
    __shared__ float s_x[NL][NV + 1];
    __shared__ float s_y[NL][NV + 1];
    __shared__ float s_v[4][P1_TH][NV + 1];
    __shared__ float s_q[NK][3][P1_TH][P1_NQ + 1];
    __shared__ float s_red[4];

    const Crop crop = s3im_crop(rect, W, H);
    const TileId tile = roi_tile<TW, P1_TH>(crop);
    const int c = tile.c, x0 = tile.bx * TW, y0 = tile.by * P1_TH, tid = threadIdx.x;
    const size_t b = ((size_t)tile.c * gridDim.y + tile.by) * gridDim.x + tile.bx;
    if (x0 >= crop.x1 || x0 + TW <= crop.x0 || y0 >= crop.y1 || y0 + P1_TH <= crop.y0) {
        if (tid == 0) partials[b] = 0.0f;          // (pass 2 never reads this tile's maps: it zeroes the gradient off the crop)
        return;
    }
    const float* xc = img + (size_t)c * H * W;
    const float* yc = gt + (size_t)c * H * W;
    {
        constexpr int NLD = (NL * NV + 255) / 256;
        float vx[NLD], vy[NLD];
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / NV, q = i % NV;
            const size_t o = (size_t)min(max(y0 + r - 5, 0), H - 1) * W + min(max(x0 + q - 2 * KH, 0), W - 1);
            vx[k] = xc[o]; vy[k] = yc[o];
        }
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / NV, q = i % NV;
            if (i < NL * NV) {
                const bool in = in_crop(crop, x0 + q - 2 * KH, y0 + r - 5);
                s_x[r][q] = in ? vx[k] : 0.0f; s_y[r][q] = in ? vy[k] : 0.0f;
            }
        }
    }
    __syncthreads();
    // vertical 11-tap of (x, y | x^2 + y^2, xy) over source rows: a thread owns P1_VR consecutive rows of one column
    for (int it = tid; it < NV * (P1_TH / P1_VR); it += 256) {
        const int q = it % NV, r0 = (it / NV) * P1_VR;
        v2f a01[P1_VR], a23[P1_VR];
#pragma unroll
        for (int j = 0; j < P1_VR; j++) { a01[j] = v2f{0.f, 0.f}; a23[j] = v2f{0.f, 0.f}; }
#pragma unroll
        for (int i = 0; i < P1_VR + 10; i++) {
            const float a = s_x[r0 + i][q], bb = s_y[r0 + i][q];
            const v2f ab = v2f{a, bb}, sx = v2f{a * a + bb * bb, a * bb};
#pragma unroll
            for (int j = 0; j < P1_VR; j++) {
                if (i - j >= 0 && i - j <= 10) {
                    const float w = win.g[i - j];
                    a01[j] = __builtin_elementwise_fma(v2f{w, w}, ab, a01[j]); a23[j] = __builtin_elementwise_fma(v2f{w, w}, sx, a23[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < P1_VR; j++) {
            s_v[0][r0 + j][q] = a01[j].x; s_v[1][r0 + j][q] = a01[j].y; s_v[2][r0 + j][q] = a23[j].x; s_v[3][r0 + j][q] = a23[j].y;
        }
    }
    __syncthreads();
    // every widened point of source column sc = x0 - KH + q (the tile's columns and KH on either side): horizontal taps, SSIM, and
    // the folded contributions Q_k = sum_r h_r(-k) D(R sc + r) that source column sc - k receives
    const int lr = tid / P1_NQ, q = tid % P1_NQ;
    const int sc = x0 - KH + q, py = y0 + lr;
    float ssim_v = 0.f;
    float acc[NK][3];
#pragma unroll
    for (int k = 0; k < NK; k++) { acc[k][0] = 0.f; acc[k][1] = 0.f; acc[k][2] = 0.f; }
    if (in_crop(crop, sc, py)) {
        v2f v01[NK], v23[NK];
#pragma unroll
        for (int k = 0; k < NK; k++) {
            v01[k] = v2f{s_v[0][lr][q + k], s_v[1][lr][q + k]}; v23[k] = v2f{s_v[2][lr][q + k], s_v[3][lr][q + k]};
        }
        const bool own = q >= KH && q < KH + TW;
        for (int r = 0; r < R; r++) {
            v2f m01 = v2f{0.f, 0.f}, m23 = v2f{0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const float w = taps.h[r][k - KH + 5];
                m01 = __builtin_elementwise_fma(v2f{w, w}, v01[k], m01); m23 = __builtin_elementwise_fma(v2f{w, w}, v23[k], m23);
            }
            // (the two variances enter only as their sum; the copies into locals keep the instruction order, as in loss.hip)
            const SsimPoint p = ssim_point(m01.x, m01.y, m23.x, m23.y);
            const float S = p.S, dS_ds1 = p.dS_ds1, dS_ds12 = p.dS_ds12, dS_dmu1 = p.dS_dmu1;
            if (own) ssim_v += S;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const float w = taps.h[r][KH - k + 5];            // h_r(-(k - KH))
                acc[k][0] = __fmaf_rn(w, dS_dmu1, acc[k][0]); acc[k][1] = __fmaf_rn(w, dS_ds1, acc[k][1]);
                acc[k][2] = __fmaf_rn(w, dS_ds12, acc[k][2]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; k++) { s_q[k][0][lr][q] = acc[k][0]; s_q[k][1][lr][q] = acc[k][1]; s_q[k][2][lr][q] = acc[k][2]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ssim_v += __shfl_xor(ssim_v, d);       // (wave.h's wave_sum here changes the kernel's SGPR count)
    if ((tid & 63) == 0) s_red[tid >> 6] = ssim_v;
    __syncthreads();
    // the folded maps of the tile's own columns: G(s) = sum_k Q_k(s + k), k = -KH .. KH in that order
    if (q < TW) {
        const int px = x0 + q;
        if (in_crop(crop, px, py)) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int k = 0; k < NK; k++) { g0 += s_q[k][0][lr][q + k]; g1 += s_q[k][1][lr][q + k]; g2 += s_q[k][2][lr][q + k]; }
            const size_t o = ((size_t)c * H + py) * W + px, plane3 = (size_t)C * H * W;
            gmap[o] = g0; gmap[plane3 + o] = g1; gmap[2 * plane3 + o] = g2;
        }
    }
    if (tid == 0) partials[b] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(256)
s3im_pass2_kernel(int C, int H, int W, int R, const float* __restrict__ img, const float* __restrict__ gt, Win win,
                  const float* __restrict__ gmap, const float* __restrict__ partials, int nblocks, float* __restrict__ dL_dimg,
                  float* __restrict__ loss_out, const int* __restrict__ rect)
{
    constexpr int NL = P2_T + 10;
    __shared__ float s_g[3][NL][P2_T + 1];
    __shared__ float s_red[4];

    const Crop crop = s3im_crop(rect, W, H);
    const TileId tile = roi_tile<P2_T, P2_T>(crop);
    const int c = tile.c, x0 = tile.bx * P2_T, y0 = tile.by * P2_T, tid = threadIdx.x;
    const bool off_crop = x0 >= crop.x1 || x0 + P2_T <= crop.x0 || y0 >= crop.y1 || y0 + P2_T <= crop.y0;    // (block-uniform)
    const float N = (float)C * crop.n_pix * (float)R;
    const size_t plane3 = (size_t)C * H * W;
    const int lx = tid % P2_T, ly0 = (tid / P2_T) * P2_VR, px = x0 + lx;
    if (!off_crop) {
        constexpr int NLD = (NL * P2_T + 255) / 256;
        float v[3][NLD];
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / P2_T, qq = i % P2_T;
            const size_t o = (size_t)c * H * W + (size_t)min(max(y0 + r - 5, 0), H - 1) * W + min(x0 + qq, W - 1);
            v[0][k] = gmap[o]; v[1][k] = gmap[plane3 + o]; v[2][k] = gmap[2 * plane3 + o];
        }
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int i = tid + 256 * k, r = i / P2_T, qq = i % P2_T;
            if (i < NL * P2_T) {
                const bool in = in_crop(crop, x0 + qq, y0 + r - 5);      // (pass 1 wrote the maps inside the crop only)
                s_g[0][r][qq] = in ? v[0][k] : 0.0f; s_g[1][r][qq] = in ? v[1][k] : 0.0f; s_g[2][r][qq] = in ? v[2][k] : 0.0f;
            }
        }
    }
    __syncthreads();
    v2f f01[P2_VR]; float f2[P2_VR];
#pragma unroll
    for (int j = 0; j < P2_VR; j++) { f01[j] = v2f{0.f, 0.f}; f2[j] = 0.f; }
    if (!off_crop) {
#pragma unroll
        for (int i = 0; i < P2_VR + 10; i++) {
            const v2f v01 = v2f{s_g[0][ly0 + i][lx], s_g[1][ly0 + i][lx]};
            const float v2 = s_g[2][ly0 + i][lx];
#pragma unroll
            for (int j = 0; j < P2_VR; j++) {
                if (i - j >= 0 && i - j <= 10) {
                    const float w = win.g[i - j];
                    f01[j] = __builtin_elementwise_fma(v2f{w, w}, v01, f01[j]); f2[j] = __fmaf_rn(w, v2, f2[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P2_VR; j++) {
        const int py = y0 + ly0 + j;
        if (px < W && py < H) {
            const size_t o = ((size_t)c * H + py) * W + px;
            float g = 0.0f;
            if (!off_crop && in_crop(crop, px, py)) g = -(f01[j].x + 2.f * img[o] * f01[j].y + gt[o] * f2[j]) / N;
            dL_dimg[o] = g;
        }
    }
    // block (0,0,0) folds pass 1's per-tile sums (written by an earlier kernel) in a fixed order
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        float a = 0.f;
        for (int i = tid; i < nblocks; i += 256) a += partials[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d);       // (not wave.h's wave_sum: it moves an instruction, and one timing row was not explained)
        if ((tid & 63) == 0) s_red[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) {
            const float s = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / N;       // (an empty crop: 0 / 0 = NaN)
            loss_out[0] = 1.0f - s; loss_out[1] = s;
        }
    }
}

// half-width in source columns of the horizontal window of a widened column: 5 for R = 1, 3 for R = 2, 2 for R = 3, 4, 1 for R >= 5
int s3im_kh(int R) { return R == 1 ? 5 : R == 2 ? 3 : R <= 4 ? 2 : 1; }

PhaseTaps make_phase_taps(const Win& win, int R)
{
    // h_r(k) = sum of g[d + 5] over d = -5..5 with floor((r + d) / R) = k; summed in double from the fp32 window, rounded once
    double h[S3_MAX_R][11] = {};
    for (int r = 0; r < R; r++)
        for (int d = -5; d <= 5; d++) {
            const int X = r + d, k = X >= 0 ? X / R : -((-X + R - 1) / R);
            h[r][k + 5] += (double)win.g[d + 5];
        }
    PhaseTaps t;
    for (int r = 0; r < S3_MAX_R; r++)
        for (int k = 0; k < 11; k++) t.h[r][k] = (float)h[r][k];
    return t;
}

size_t s3im_partials(int C, int H, int W, int tw) { return (size_t)((W + tw - 1) / tw) * ((H + P1_TH - 1) / P1_TH) * C; }

template <int KH>
void launch_s3im(int C, int H, int W, int R, const float* image, const float* gt, const int* rect, float* loss_out, float* dL_dimage,
                 float* gmap, float* partials, const Win& win, const PhaseTaps& taps, hipStream_t s)
{
    constexpr int TW = p1_tw<KH>();
    const dim3 g1((W + TW - 1) / TW, (H + P1_TH - 1) / P1_TH, C), g2((W + P2_T - 1) / P2_T, (H + P2_T - 1) / P2_T, C);
    hipLaunchKernelGGL((s3im_pass1_kernel<KH>), g1, dim3(256), 0, s, C, H, W, R, image, gt, win, taps, gmap, partials, rect);
    hipLaunchKernelGGL(s3im_pass2_kernel, g2, dim3(256), 0, s, C, H, W, R, image, gt, win, gmap, partials, (int)(g1.x * g1.y * g1.z),
                       dL_dimage, loss_out, rect);
}

}  // anonymous namespace
}  // namespace moss

using namespace moss;

extern "C" size_t moss_s3im_workspace_bytes(int C, int H, int W)
{
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    // (the per-tile sums of the narrowest pass-1 tile, R = 1's: the same workspace serves every R)
    return align_up(3 * (size_t)C * H * W * 4) + align_up(s3im_partials(C, H, W, p1_tw<5>()) * 4);
}

extern "C" int moss_s3im_loss(int C, int H, int W, const float* image, const float* gt, const int* rect, int repeat, float* loss_out,
                              float* dL_dimage, char* workspace, size_t workspace_bytes, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return invalid_arg("moss_s3im_loss", "C, H and W must be positive");
    if (!image || !gt || !loss_out || !dL_dimage || !workspace) return invalid_arg("moss_s3im_loss", "a required pointer is NULL");
    if (repeat < 1 || repeat > S3_MAX_R) return invalid_arg("moss_s3im_loss", "repeat must be 1..16");
    if (workspace_bytes < moss_s3im_workspace_bytes(C, H, W)) return invalid_arg("moss_s3im_loss", "workspace too small (moss_s3im_workspace_bytes)");
    static const Win win = make_window();
    static PhaseTaps taps_by_r[S3_MAX_R + 1];
    static bool taps_ready = [] { for (int r = 1; r <= S3_MAX_R; r++) taps_by_r[r] = make_phase_taps(win, r); return true; }();
    (void)taps_ready;
    char* p = workspace;
    float* gmap = carve<float>(p, 3 * (size_t)C * H * W);
    float* partials = carve<float>(p, s3im_partials(C, H, W, p1_tw<5>()));
    hipStream_t s = (hipStream_t)stream;
    const PhaseTaps& t = taps_by_r[repeat];
    switch (s3im_kh(repeat)) {
    case 5: launch_s3im<5>(C, H, W, repeat, image, gt, rect, loss_out, dL_dimage, gmap, partials, win, t, s); break;
    case 3: launch_s3im<3>(C, H, W, repeat, image, gt, rect, loss_out, dL_dimage, gmap, partials, win, t, s); break;
    case 2: launch_s3im<2>(C, H, W, repeat, image, gt, rect, loss_out, dL_dimage, gmap, partials, win, t, s); break;
    default: launch_s3im<1>(C, H, W, repeat, image, gt, rect, loss_out, dL_dimage, gmap, partials, win, t, s); break;
    }
    return launch_status("moss_s3im_loss");
}
