// view_images.hip -- a view's ground truth from its raw image and mask, and its way back to float32 (include/moss_raster.h
// moss_view_images_prepare / moss_view_images_load): the image path of MOSS's dataset readers (scene/dataset_readers.py:613-654,
// :361-407, :830-868 and utils/general_utils.py:22-28) without OpenCV.
//     prepare:  interleaved (H0,W0,3) bytes + (H0,W0) mask bytes + K, D  ->  planar (3,H,W) bytes + (H,W) mask bytes, H = H0 / scale
//     load:     those bytes / 255.f                                      ->  (3,H,W) and (1,H,W) float32
// The contract -- the float64 map, its quantisation to 1/32 pixel, the float32 bilinear taps, the two mask rules, the matte, the box
// mean and the truncation -- is stated in the header; this file is compiled with -ffp-contract=off (moss_amd/build.py), so every
// operation below rounds on its own exactly as written.
//
// prepare: one thread per OUTPUT pixel, 256 per workgroup, blockIdx.y = the view; scale^2 samples per thread.
//   byte / 255.f: a 256-entry table in LDS, filled by the workgroup with the correctly rounded division (12-16 lookups per sample
//           instead of as many divisions).
//   loads:  the two taps of a row are 6 consecutive bytes of the interleaved image: where the view's `rgb` is 4-byte aligned -- the
//           entry point checks and passes a bit per view -- they come as two aligned dwords (one 8-byte load, plus one byte load
//           when the six start at the last byte of a dword; not taken where the 8 bytes would end beyond the image), else byte by
//           byte.  The two mask taps come out of one aligned dword
//           when they lie in one and `mask` is 4-byte aligned.  A tap outside the image is never addressed.
//   stores: when H*W is a multiple of 4 and the view's outputs are 4-byte aligned, four neighbouring lanes' bytes of a plane are
//           gathered in the first of them and stored as one dword; else every lane stores its own byte.  Exactly 4*H*W bytes.
#include "common.h"

namespace moss {

namespace {

constexpr int MAX_VIEWS = 8;

struct Lens { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };

struct Views {
    const unsigned char* rgb[MAX_VIEWS];
    const unsigned char* mask[MAX_VIEWS];
    unsigned char* gt[MAX_VIEWS];
    unsigned char* bkgd[MAX_VIEWS];
    Lens lens[MAX_VIEWS];
};

struct __attribute__((aligned(4))) Dwords2 { uint32_t a, b; };

// The bytes of the taps (ix, yy) and (ix + 1, yy): c0 / c1 the colours, m0 / m1 the mask bytes; 0 for a tap outside the image.
__device__ __forceinline__ void row_taps(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ msk, int H0, int W0,
                                         int yy, int ix, bool wide_rgb, bool wide_mask, uint32_t (&c0)[3], uint32_t (&c1)[3],
                                         uint32_t& m0, uint32_t& m1)
{
    c0[0] = c0[1] = c0[2] = c1[0] = c1[1] = c1[2] = m0 = m1 = 0u;
    const bool row = yy >= 0 && yy < H0;
    const bool in0 = row && ix >= 0 && ix < W0, in1 = row && ix + 1 >= 0 && ix + 1 < W0;
    if (!in0 && !in1) return;
    const int total = H0 * W0;                                  // (3 * total < 2^31: the entry point refuses more)
    const int px = yy * W0 + (in0 ? ix : ix + 1);               // the first tap that exists
    const int off = 3 * px;
    if (in0 && in1) {
        // the 6 bytes start 0..3 bytes into an aligned dword: from 0..2 they lie inside that dword and the next; from 3 the first is
        // read on its own and the other five lie inside the next two dwords
        const int o = off & 3, aoff = o == 3 ? off + 1 : off - o;
        if (wide_rgb && aoff + 8 <= 3 * total) {
            const Dwords2 d = *reinterpret_cast<const Dwords2*>(rgb + aoff);
            uint64_t v = ((uint64_t)d.b << 32) | d.a;
            v = o == 3 ? (v << 8) | rgb[off] : v >> (8 * o);
            c0[0] = (uint32_t)v & 0xffu; c0[1] = (uint32_t)(v >> 8) & 0xffu; c0[2] = (uint32_t)(v >> 16) & 0xffu;
            c1[0] = (uint32_t)(v >> 24) & 0xffu; c1[1] = (uint32_t)(v >> 32) & 0xffu; c1[2] = (uint32_t)(v >> 40) & 0xffu;
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) { c0[c] = rgb[off + c]; c1[c] = rgb[off + 3 + c]; }
        }
        const int om = px & 3, apx = px & ~3;
        if (wide_mask && om <= 2 && apx + 4 <= total) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(msk + apx) >> (8 * om);
            m0 = w & 0xffu; m1 = (w >> 8) & 0xffu;
        } else {
            m0 = msk[px]; m1 = msk[px + 1];
        }
    } else if (in0) {
#pragma unroll
        for (int c = 0; c < 3; c++) c0[c] = rgb[off + c];
        m0 = msk[px];
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) c1[c] = rgb[off + c];
        m1 = msk[px];
    }
}

// One full-resolution sample at the normalised coordinates (x, y): its matted colour and its mask value m.
template <int MODE>
__device__ __forceinline__ void sample(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ msk, int H0, int W0,
                                       const Lens& L, double x, double y, bool wide_rgb, bool wide_mask, const float* lut,
                                       float background, float (&colour)[3], float& m)
{
    // 1. the map
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
    const double kr = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
    const double xd = (x * kr + L.p1 * xy2) + L.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + L.p1 * (r2 + 2.0 * y2)) + L.p2 * xy2;
    const double su = L.fx * xd + L.cx, sv = L.fy * yd + L.cy;
    const double iu = rint(su * 32.0), iv = rint(sv * 32.0);
    const bool finite = fabs(iu) < 1073741824.0 && fabs(iv) < 1073741824.0;        // (false for NaN and inf)
    int ix = -2, iy = -2, ax = 0, ay = 0;                                           // every tap outside
    if (finite) {
        const int qu = (int)iu, qv = (int)iv;
        ix = qu >> 5; ax = qu & 31; iy = qv >> 5; ay = qv & 31;
    }
    // 2. the taps
    uint32_t c00[3], c01[3], c10[3], c11[3], m00, m01, m10, m11;
    row_taps(rgb, msk, H0, W0, iy, ix, wide_rgb, wide_mask, c00, c01, m00, m01);
    row_taps(rgb, msk, H0, W0, iy + 1, ix, wide_rgb, wide_mask, c10, c11, m10, m11);
    // 3. the weights (exact in float32: multiples of 1/1024 up to 1)
    const float fx1 = (float)ax / 32.0f, fy1 = (float)ay / 32.0f, fx0 = 1.0f - fx1, fy0 = 1.0f - fy1;
    const float w00 = fy0 * fx0, w01 = fy0 * fx1, w10 = fy1 * fx0, w11 = fy1 * fx1;
    bool foreground;
    if (MODE == 0) {                                                                // 4. round
        const int s = (m00 != 0u ? (32 - ax) * (32 - ay) : 0) + (m01 != 0u ? ax * (32 - ay) : 0) + (m10 != 0u ? (32 - ax) * ay : 0)
                    + (m11 != 0u ? ax * ay : 0);
        foreground = s >= 512;
        m = foreground ? 1.0f : 0.0f;
    } else {                                                                        // 5. any
        m = ((lut[m00] * w00 + lut[m01] * w01) + lut[m10] * w10) + lut[m11] * w11;
        foreground = m != 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = ((lut[c00[c]] * w00 + lut[c01[c]] * w01) + lut[c10[c]] * w10) + lut[c11[c]] * w11;
        colour[c] = foreground ? v : background;                                    // 6. the matte
    }
}

template <int SCALE, int MODE>
__global__ void __launch_bounds__(256)
view_images_prepare_kernel(Views F, int H0, int W0, float background, uint32_t wide_rgb, uint32_t wide_mask, uint32_t packed_out)
{
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)threadIdx.x / 255.0f;            // (256 threads: the launch's block size)
    __syncthreads();
    const int view = (int)blockIdx.y;
    // this view's arguments (static indices: a run-time index into the argument struct would be copied to private memory first)
    const unsigned char* rgb = nullptr; const unsigned char* msk = nullptr; unsigned char* gt = nullptr; unsigned char* bk = nullptr;
    Lens L = F.lens[0];
#pragma unroll
    for (int v = 0; v < MAX_VIEWS; v++)
        if (v == view) { rgb = F.rgb[v]; msk = F.mask[v]; gt = F.gt[v]; bk = F.bkgd[v]; L = F.lens[v]; }
    const bool wr = (wide_rgb >> view) & 1u, wm = (wide_mask >> view) & 1u;
    const int W = W0 / SCALE, n = (H0 / SCALE) * W;
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = p < n;
    uint32_t q[4] = {0u, 0u, 0u, 0u};                          // R, G, B and mask bytes of this pixel
    if (live) {
        const int i = p / W, j = p - i * W;
        double xs[SCALE];
#pragma unroll
        for (int d = 0; d < SCALE; d++) xs[d] = ((double)(SCALE * j + d) - L.cx) / L.fx;
        float m_first = 0.0f;
        // the tree sum of sample row dy: the sample, the pair, or the pair of pairs
        auto row_sum = [&](int dy, float (&out)[3]) {
            const double y = ((double)(SCALE * i + dy) - L.cy) / L.fy;
            float s[SCALE][3];
#pragma unroll
            for (int dx = 0; dx < SCALE; dx++) {
                float m;
                sample<MODE>(rgb, msk, H0, W0, L, xs[dx], y, wr, wm, lut, background, s[dx], m);
                if (dx == 0 && dy == 0) m_first = m;
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if constexpr (SCALE == 1) out[c] = s[0][c];
                else if constexpr (SCALE == 2) out[c] = s[0][c] + s[1][c];
                else out[c] = (s[0][c] + s[1][c]) + (s[2][c] + s[3][c]);
            }
        };
        float v[3];
        if (SCALE == 1) {
            row_sum(0, v);
        } else {
            // rows 0 + 1, then (scale 4) rows 2 + 3 and the sum of the two halves; the scale-4 loop stays rolled: 16 samples unrolled
            // would take every vector register there is
            float half[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int h = 0; h < SCALE / 2; h++) {
                float r0[3], r1[3];
                row_sum(2 * h, r0);
                row_sum(2 * h + 1, r1);
#pragma unroll
                for (int c = 0; c < 3; c++) half[c] = h == 0 ? r0[c] + r1[c] : half[c] + (r0[c] + r1[c]);
            }
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = half[c] * (SCALE == 2 ? 0.25f : 0.0625f);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) q[c] = (uint32_t)(int)(v[c] * 255.0f);   // 0 <= v <= 1: the conversion truncates
        q[3] = (uint32_t)(int)(m_first * 255.0f);
    }
    if ((packed_out >> view) & 1u) {                           // (uniform; then n % 4 == 0: a quad of lanes is live or dead as a whole)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t t = q[c] | ((uint32_t)__shfl_down((int)q[c], 1) << 8);
            t |= (uint32_t)__shfl_down((int)t, 2) << 16;
            if (live && (threadIdx.x & 3u) == 0u)
                *reinterpret_cast<uint32_t*>((c < 3 ? gt + (size_t)c * n : bk) + p) = t;
        }
    } else if (live) {
#pragma unroll
        for (int c = 0; c < 3; c++) gt[(size_t)c * n + p] = (unsigned char)q[c];
        bk[p] = (unsigned char)q[3];
    }
}

// load: one thread per four bytes -- the groups of gt_u8 first, then those of bkgd_u8.
__global__ void __launch_bounds__(256)
view_images_load_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ bk, float* __restrict__ gt_image,
                        float* __restrict__ bkgd_mask, int n3 /* 3 H W */, int n /* H W */, int groups3, int wide_gt, int wide_bk)
{
    int g = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool first = g < groups3;
    if (!first) g -= groups3;
    const unsigned char* src = first ? gt : bk;
    float* dst = first ? gt_image : bkgd_mask;
    const int len = first ? n3 : n;
    const int e0 = 4 * g;
    if (e0 >= len) return;
    const int count = min(4, len - e0);
    if (count == 4 && (first ? wide_gt : wide_bk)) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(src + e0);
        float4 o;
        o.x = (float)(w & 0xffu) / 255.0f; o.y = (float)((w >> 8) & 0xffu) / 255.0f;
        o.z = (float)((w >> 16) & 0xffu) / 255.0f; o.w = (float)(w >> 24) / 255.0f;
        *reinterpret_cast<float4*>(dst + e0) = o;
    } else {
        for (int k = 0; k < count; k++) dst[e0 + k] = (float)src[e0 + k] / 255.0f;
    }
}

template <int SCALE>
void launch_prepare(int mode, dim3 grid, hipStream_t s, const Views& F, int H0, int W0, float background, uint32_t wide_rgb,
                    uint32_t wide_mask, uint32_t packed_out)
{
    if (mode == 0)
        hipLaunchKernelGGL((view_images_prepare_kernel<SCALE, 0>), grid, dim3(256), 0, s, F, H0, W0, background, wide_rgb, wide_mask, packed_out);
    else
        hipLaunchKernelGGL((view_images_prepare_kernel<SCALE, 1>), grid, dim3(256), 0, s, F, H0, W0, background, wide_rgb, wide_mask, packed_out);
}

}  // anonymous namespace
}  // namespace moss

using namespace moss;

extern "C" int moss_view_images_prepare(const moss_view_images_prepare_args* a, void* stream)
{
    const char* who = "moss_view_images_prepare";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->num_views < 1 || a->num_views > MAX_VIEWS) return invalid_arg(who, "num_views outside 1..8");
    if (a->H0 <= 0 || a->W0 <= 0) return invalid_arg(who, "H0 <= 0 or W0 <= 0");
    if ((long long)a->H0 * a->W0 * 3 >= 0x80000000LL) return invalid_arg(who, "H0 * W0 * 3 must be < 2^31");
    if (a->scale != 1 && a->scale != 2 && a->scale != 4) return invalid_arg(who, "scale is none of 1, 2, 4");
    if (a->H0 % a->scale != 0 || a->W0 % a->scale != 0) return invalid_arg(who, "scale does not divide H0 and W0");
    if (a->background != 0 && a->background != 1) return invalid_arg(who, "background is neither 0 nor 1");
    if (a->mask_mode != 0 && a->mask_mode != 1) return invalid_arg(who, "mask_mode is neither 0 (round) nor 1 (any)");
    const int n = (a->H0 / a->scale) * (a->W0 / a->scale);
    Views F;
    uint32_t wide_rgb = 0, wide_mask = 0, packed_out = 0;
    for (int v = 0; v < MAX_VIEWS; v++) {
        const int u = v < a->num_views ? v : 0;                // (the unused slots repeat view 0: never selected)
        if (v < a->num_views) {
            if (!a->rgb[v] || !a->mask[v]) return invalid_arg(who, "null rgb or mask of a view");
            if (!a->gt_u8[v] || !a->bkgd_u8[v]) return invalid_arg(who, "null gt_u8 or bkgd_u8 of a view");
            if (a->K[v][1] != 0.0) return invalid_arg(who, "K[0][1] (skew) of a view is not 0");
            if (!(a->K[v][0] > 0.0) || !(a->K[v][4] > 0.0)) return invalid_arg(who, "fx or fy of a view is not positive");
            // what the kernel's wide accesses rely on, and nothing more
            if (((uintptr_t)a->rgb[v] & 3u) == 0) wide_rgb |= 1u << v;
            if (((uintptr_t)a->mask[v] & 3u) == 0) wide_mask |= 1u << v;
            if (n % 4 == 0 && ((uintptr_t)a->gt_u8[v] & 3u) == 0 && ((uintptr_t)a->bkgd_u8[v] & 3u) == 0) packed_out |= 1u << v;
        }
        F.rgb[v] = a->rgb[u]; F.mask[v] = a->mask[u]; F.gt[v] = a->gt_u8[u]; F.bkgd[v] = a->bkgd_u8[u];
        F.lens[v] = Lens{a->K[u][0], a->K[u][4], a->K[u][2], a->K[u][5], a->D[u][0], a->D[u][1], a->D[u][2], a->D[u][3], a->D[u][4]};
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)a->num_views);
    const float background = (float)a->background;
    if (a->scale == 1) launch_prepare<1>(a->mask_mode, grid, s, F, a->H0, a->W0, background, wide_rgb, wide_mask, packed_out);
    else if (a->scale == 2) launch_prepare<2>(a->mask_mode, grid, s, F, a->H0, a->W0, background, wide_rgb, wide_mask, packed_out);
    else launch_prepare<4>(a->mask_mode, grid, s, F, a->H0, a->W0, background, wide_rgb, wide_mask, packed_out);
    return launch_status(who);
}

extern "C" int moss_view_images_load(const moss_view_images_load_args* a, void* stream)
{
    const char* who = "moss_view_images_load";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->H <= 0 || a->W <= 0) return invalid_arg(who, "H <= 0 or W <= 0");
    if ((long long)a->H * a->W * 3 >= 0x80000000LL) return invalid_arg(who, "H * W * 3 must be < 2^31");
    if (!a->gt_u8 || !a->bkgd_u8) return invalid_arg(who, "null gt_u8 or bkgd_u8");
    if (!a->gt_image || !a->bkgd_mask) return invalid_arg(who, "null gt_image or bkgd_mask");
    if (((uintptr_t)a->gt_image & 3u) || ((uintptr_t)a->bkgd_mask & 3u)) return invalid_arg(who, "gt_image or bkgd_mask not 4-byte aligned");
    const int n = a->H * a->W, n3 = 3 * n;
    const int groups3 = (n3 + 3) / 4, groups = groups3 + (n + 3) / 4;
    const int wide_gt = ((uintptr_t)a->gt_u8 & 3u) == 0 && ((uintptr_t)a->gt_image & 15u) == 0;
    const int wide_bk = ((uintptr_t)a->bkgd_u8 & 3u) == 0 && ((uintptr_t)a->bkgd_mask & 15u) == 0;
    hipLaunchKernelGGL(view_images_load_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->gt_u8,
                       a->bkgd_u8, a->gt_image, a->bkgd_mask, n3, n, groups3, wide_gt, wide_bk);
    return launch_status(who);
}
