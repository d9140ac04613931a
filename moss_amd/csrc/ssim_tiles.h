// ssim_tiles.h -- what the SSIM-stencil kernels (loss.hip, s3im.hip) share: the 11-tap window, the crop read from device memory and
// its clipping rules, and the tile orders (XCD-aware; crop-first for the ROI instantiations).  Internal to each translation unit.
#pragma once
#include "common.h"

namespace moss {

namespace {

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
struct TileId { int bx, by, c; };
__device__ __forceinline__ TileId xcd_tile()
{
    const int total = (int)(gridDim.x * gridDim.y * gridDim.z);
    const int lin = (int)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
    const int q = total / 8, r = total % 8, xcd = lin % 8, j = lin / 8;
    const int t = xcd * q + min(xcd, r) + j;
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
