// ssim_tiles.h -- what the SSIM-stencil kernels (loss.hip, s3im.hip, metrics.hip) share: the 11-tap window, the crop read from device
// memory and its clipping rules, the tile orders (XCD-aware, by grid or by linear id; crop-first for the ROI instantiations), the
// 32 x 32 tile's constants and the closing step of its block sums (loss.hip, metrics.hip), and SSIM with its derivatives at a point
// (loss.hip, s3im.hip).  The four-moment filter and the wave sums of the tile kernels are still written out in loss.hip and in
// metrics.hip: each was tried as a shared function on its own, profiles/shared_device_code_notes.md section 5 has the numbers.
// Internal to each translation unit.
#pragma once
#include "common.h"

namespace moss {

namespace {

constexpr int LT = 32;              // tile edge: 32 x 32 outputs per 256-thread workgroup
constexpr int HALO = 5;             // window 11
constexpr int LP = LT + 2 * HALO;   // 42
constexpr int SEG = 8;              // outputs per thread in the horizontal pass (a run of 8 in one row: 18 inputs)
constexpr int VR = 4;               // outputs per thread in the vertical pass (4 consecutive rows of one column: 14 inputs)
static_assert(LT % SEG == 0 && (LT / SEG) * LP <= 256 && LT * (LT / VR) == 256, "work split of a 256-thread workgroup");

typedef float v2f __attribute__((ext_vector_type(2)));

struct Win { float g[11]; };

// the crop [x0, x1) x [y0, y1) clipped to the image, its pixel count and the number of `bound` pixels (= the crop's when there is no mask)
struct Crop { int x0, y0, x1, y1; float n_pix, n_bound; };
__device__ __forceinline__ Crop load_crop(const int* __restrict__ rect, int W, int H, bool has_bound)
{
    Crop r;
    const int x = rect[0], y = rect[1], w = max(rect[2], 0), h = max(rect[3], 0);
    const long long xe = (long long)x + w, ye = (long long)y + h;     // (the rectangle's far edges, before clipping: x may be negative)
    r.x0 = min(max(x, 0), W); r.y0 = min(max(y, 0), H);
    r.x1 = (int)min(max(xe, (long long)r.x0), (long long)W); r.y1 = (int)min(max(ye, (long long)r.y0), (long long)H);
    r.n_pix = (float)(r.x1 - r.x0) * (float)(r.y1 - r.y0);
    r.n_bound = has_bound ? (float)rect[4] : r.n_pix;
    return r;
}
__device__ __forceinline__ bool in_crop(const Crop& r, int x, int y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }


// XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs (linear id % 8), each with its own L2: with the natural
// order, a tile's four neighbours -- which re-read its 5-pixel halo -- run on four other XCDs and every halo is fetched from HBM
// again (PMC: 39 / 52 MB per launch against 16 / 25 MB of distinct data).  Here XCD k takes the k-th contiguous eighth of the
// (channel, row, column) tile sequence, so neighbouring tiles share an L2.
// (the place in that sequence of workgroup `lin` of `total`)
__device__ __forceinline__ int xcd_order(int lin, int total)
{
    const int q = total / 8, r = total % 8, xcd = lin % 8, j = lin / 8;
    return xcd * q + min(xcd, r) + j;
}
struct TileId { int bx, by, c; };
__device__ __forceinline__ TileId xcd_tile()
{
    const int total = (int)(gridDim.x * gridDim.y * gridDim.z);
    const int lin = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
    const int t = xcd_order(lin, total);
    TileId id;
    id.bx = t % (int)gridDim.x; id.by = (t / (int)gridDim.x) % (int)gridDim.y; id.c = t / (int)(gridDim.x * gridDim.y);
    return id;
}

// The crop instantiations: the tiles that meet the crop FIRST.  Workgroups are dispatched in linear-id order as slots free up; at 1024 x 1024
// the grid takes three residency rounds and, in image order, the crop's tiles (a person in the middle of the frame) are handed out behind
// the empty ones in front of them.  Here XCD x (linear id % 8) is dealt, in its turns j = id / 8, first the x-th contiguous eighth of the
// crop's tiles -- (channel, row, column) order inside the crop's tile rectangle: neighbours still share an L2 -- and then its share of the
// tiles off the crop (which leave at once).
template <int TW, int TH>        // (the tile's width and height in pixels)
__device__ __forceinline__ TileId roi_tile(const Crop& cr)
{
    const int gx = (int)gridDim.x, gy = (int)gridDim.y, C = (int)gridDim.z;
    const int total = gx * gy * C;
    const int lin = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
    const bool some = cr.x1 > cr.x0 && cr.y1 > cr.y0;
    const int tx0 = cr.x0 / TW, ty0 = cr.y0 / TH;
    const int ncx = some ? (cr.x1 - 1) / TW - tx0 + 1 : 0, ncy = some ? (cr.y1 - 1) / TH - ty0 + 1 : 0;
    const int n_crop = ncx * ncy, n_in = n_crop * C;
    const int x = lin % 8, j = lin / 8;
    const int q = n_in / 8, r = n_in % 8, qt = total / 8, rt = total % 8;
    const int cnt = q + (x < r ? 1 : 0);                     // crop tiles dealt to this XCD
    TileId id;
    if (j < cnt) {
        const int ci = x * q + min(x, r) + j;
        const int rem = ci % n_crop;
        id.c = ci / n_crop; id.by = ty0 + rem / ncx; id.bx = tx0 + rem % ncx;
        return id;
    }
    // the (oi)-th tile off the crop, in (channel, row, column) order: the rows above the crop, the crop's rows without its columns, the rows below
    const int oi = (x * qt + min(x, rt)) - (x * q + min(x, r)) + (j - cnt);
    const int n_off = gx * gy - n_crop;                      // per channel (> 0 here: some block is left over for this branch)
    id.c = oi / n_off;
    int k = oi % n_off;
    const int above = ty0 * gx, side = gx - ncx;
    if (!some || k < above) { id.by = k / gx; id.bx = k % gx; return id; }
    k -= above;
    if (side > 0 && k < ncy * side) {
        const int cc = k % side;
        id.by = ty0 + k / side; id.bx = cc < tx0 ? cc : cc + ncx;
        return id;
    }
    k -= ncy * side;
    id.by = ty0 + ncy + k / gx; id.bx = k % gx;
    return id;
}

// SSIM at a point from its four windowed moments, and its total derivatives w.r.t. the three filtered moments that depend on x:
// E[x], E[x^2], E[xy] (sigma1^2 = E[x^2] - mu1^2, sigma12 = E[xy] - mu1 mu2)
struct SsimPoint { float S, dS_dmu1, dS_ds1, dS_ds12; };
__device__ __forceinline__ SsimPoint ssim_point(float mu1, float mu2, float ess /* E[x^2 + y^2] */, float exy)
{
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float s12 = exy - mu12;
    // sigma1^2 + sigma2^2 = E[x^2 + y^2] - mu1^2 - mu2^2 (utils/loss_utils.py:73-75 forms the two variances and adds them)
    const float a1 = 2.f * mu12 + C1, a2 = 2.f * s12 + C2, b1 = mu1_sq + mu2_sq + C1, b2 = (ess - mu1_sq - mu2_sq) + C2;
    // (hardware reciprocals, ~1 ulp: these files are compiled with correctly rounded division, ten instructions apiece, and the
    // four quotients per pixel-channel were an eighth of the loss kernel's vector instructions; b1 >= C1, b2 ~ C2 + variances)
    const float rb1 = __builtin_amdgcn_rcpf(b1), rb2 = __builtin_amdgcn_rcpf(b2), inv = rb1 * rb2;
    SsimPoint p;
    p.S = a1 * a2 * inv;
    // partial derivatives of S w.r.t. (mu1 | sigma1^2 | sigma12), then the total derivative w.r.t. E[x]
    p.dS_ds1 = -p.S * rb2;
    p.dS_ds12 = 2.f * a1 * inv;
    p.dS_dmu1 = 2.f * mu2 * a2 * inv - p.S * 2.f * mu1 * rb1 + p.dS_ds1 * (-2.f * mu1) + p.dS_ds12 * (-mu2);
    return p;
}

// the workgroup's k-th sum from its four waves' (s_red[k][wave], staged before a barrier), in a fixed order
__device__ __forceinline__ float block_sum3(const float (&s_red)[3][4], int k) { return (s_red[k][0] + s_red[k][1]) + (s_red[k][2] + s_red[k][3]); }

Win make_window()
{
    // utils/loss_utils.py:47-49: gauss = Tensor([exp(-(x-5)^2 / (2*1.5^2))]) / sum, evaluated in fp32 like torch.Tensor
    Win w; float sum = 0.f;
    for (int i = 0; i < 11; i++) { w.g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += w.g[i]; }
    for (int i = 0; i < 11; i++) w.g[i] /= sum;
    return w;
}

}  // anonymous namespace
}  // namespace moss
