// present.hip -- float32 frames to 8-bit pixels, up to eight views per launch (include/moss_raster.h moss_frames_to_u8): what
// render_ZJU.py:83-84 does through torchvision's save_image and train_ZJU.py:75 for the viewer, as one streaming kernel.
//     planar (3,H,W) float32 [+ (H,W) float32 alpha] [+ (H,W) byte mask]  ->  interleaved (H,W,3|4) bytes
// Per element, in float32, every operation rounded on its own (no FMA):
//     nearest:   trunc(min(max(x * 255 + 0.5, 0), 255))        save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
//     truncate:  trunc(min(max(x, 0), 1) * 255)                train_ZJU.py:75
// NaN gives 0 in both.  Where the mask is != 1 the colour is `fill` BEFORE it is quantised; alpha is quantised by the same rule and
// never filled.
//
// One thread takes four consecutive pixels of one view: 12-16 bytes read and 3-4 written per pixel, nothing is read twice.
//   loads:  when H*W is a multiple of 4 and the view's image (alpha) is 16-byte and its mask 4-byte aligned -- the entry point checks
//           and passes a bit per view -- each plane is read as one float4 and the mask as one dword; else element by element.
//   stores: the 12 (RGB) or 16 (RGBA) bytes of a full group are packed into 3 or 4 dwords and stored as such when the view's `out` is
//           4-byte aligned (group g starts 12 g or 16 g bytes in: dword alignment is all that holds, and all that is assumed); else,
//           and for the last, partial group of a frame, byte by byte.  Exactly H*W*channels bytes are written, at any address.
#include "common.h"

namespace moss {

namespace {

constexpr int MAX_VIEWS = 8;
constexpr int GROUP = 4;                              // pixels per thread

struct Frames {
    const float* image[MAX_VIEWS];
    const float* alpha[MAX_VIEWS];
    const unsigned char* bound[MAX_VIEWS];
    unsigned char* out[MAX_VIEWS];
};

struct __attribute__((aligned(4))) Dwords3 { uint32_t a, b, c; };
struct __attribute__((aligned(4))) Dwords4 { uint32_t a, b, c, d; };

template <int ROUNDING>
__device__ __forceinline__ uint32_t quantise(float x)
{
    float t;
    if (ROUNDING == 0) {
        t = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
        t = t > 0.0f ? t : 0.0f;                       // (NaN > 0 is false: NaN -> 0)
        t = t < 255.0f ? t : 255.0f;
    } else {
        t = x > 0.0f ? x : 0.0f;
        t = t < 1.0f ? t : 1.0f;
        t = __fmul_rn(t, 255.0f);
    }
    return (uint32_t)(int)t;                           // 0 <= t <= 255: the conversion truncates
}

template <int CH, int ROUNDING>
__global__ void __launch_bounds__(256)
frames_to_u8_kernel(Frames F, long long n /* H * W */, float fill, uint32_t wide_in, uint32_t wide_out)
{
    const int view = (int)blockIdx.y;
    // this view's pointers (static indices: a run-time index into the argument struct would be copied to private memory first)
    const float* img = nullptr; const float* al = nullptr; const unsigned char* bd = nullptr; unsigned char* out = nullptr;
#pragma unroll
    for (int v = 0; v < MAX_VIEWS; v++)
        if (v == view) { img = F.image[v]; al = F.alpha[v]; bd = F.bound[v]; out = F.out[v]; }
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * GROUP;
    if (p0 >= n) return;
    const int count = (int)min((long long)GROUP, n - p0);

    float r[GROUP], g[GROUP], b[GROUP], a[GROUP];
    uint32_t keep[GROUP];
    if ((wide_in >> view) & 1u) {                      // (then n % 4 == 0: every group is full)
        const float4 vr = *reinterpret_cast<const float4*>(img + p0);
        const float4 vg = *reinterpret_cast<const float4*>(img + n + p0);
        const float4 vb = *reinterpret_cast<const float4*>(img + 2 * n + p0);
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
        if (CH == 4) va = *reinterpret_cast<const float4*>(al + p0);
        const uint32_t m = bd != nullptr ? *reinterpret_cast<const uint32_t*>(bd + p0) : 0x01010101u;
        r[0] = vr.x; r[1] = vr.y; r[2] = vr.z; r[3] = vr.w;
        g[0] = vg.x; g[1] = vg.y; g[2] = vg.z; g[3] = vg.w;
        b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
        a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
#pragma unroll
        for (int k = 0; k < GROUP; k++) keep[k] = ((m >> (8 * k)) & 0xffu) == 1u;
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            const long long p = p0 + (k < count ? k : 0);          // (a clamped address: the loads of a partial group stay inside)
            r[k] = img[p]; g[k] = img[n + p]; b[k] = img[2 * n + p];
            a[k] = CH == 4 ? al[p] : 0.f;
            keep[k] = bd != nullptr ? (bd[p] == (unsigned char)1) : 1u;
        }
    }
    uint32_t q[GROUP][4];
#pragma unroll
    for (int k = 0; k < GROUP; k++) {
        q[k][0] = quantise<ROUNDING>(keep[k] ? r[k] : fill);
        q[k][1] = quantise<ROUNDING>(keep[k] ? g[k] : fill);
        q[k][2] = quantise<ROUNDING>(keep[k] ? b[k] : fill);
        q[k][3] = CH == 4 ? quantise<ROUNDING>(a[k]) : 0u;
    }
    unsigned char* o = out + (size_t)p0 * CH;
    if (count == GROUP && ((wide_out >> view) & 1u)) {
        if (CH == 4) {
            Dwords4 d;
            d.a = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[0][3] << 24);
            d.b = q[1][0] | (q[1][1] << 8) | (q[1][2] << 16) | (q[1][3] << 24);
            d.c = q[2][0] | (q[2][1] << 8) | (q[2][2] << 16) | (q[2][3] << 24);
            d.d = q[3][0] | (q[3][1] << 8) | (q[3][2] << 16) | (q[3][3] << 24);
            *reinterpret_cast<Dwords4*>(o) = d;
        } else {
            Dwords3 d;                                 // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            d.a = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
            d.b = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
            d.c = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
            *reinterpret_cast<Dwords3*>(o) = d;
        }
    } else {
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            if (k < count) {
#pragma unroll
                for (int c = 0; c < CH; c++) o[k * CH + c] = (unsigned char)q[k][c];
            }
        }
    }
}

}  // anonymous namespace
}  // namespace moss

using namespace moss;

extern "C" int moss_frames_to_u8(const moss_frames_to_u8_args* a, void* stream)
{
    const char* who = "moss_frames_to_u8";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->num_views < 1 || a->num_views > MAX_VIEWS) return invalid_arg(who, "num_views outside 1..8");
    if (a->H <= 0 || a->W <= 0) return invalid_arg(who, "H <= 0 or W <= 0");
    if (a->channels_out != 3 && a->channels_out != 4) return invalid_arg(who, "channels_out is neither 3 nor 4");
    if (a->rounding != 0 && a->rounding != 1) return invalid_arg(who, "rounding is neither 0 (nearest) nor 1 (truncate)");
    const long long n = (long long)a->H * a->W;
    const long long blocks = ((n + GROUP - 1) / GROUP + 255) / 256;
    if (blocks > 0x7fffffffLL) return invalid_arg(who, "H * W beyond one grid");
    Frames F;
    uint32_t wide_in = 0, wide_out = 0;
    for (int v = 0; v < MAX_VIEWS; v++) {
        const bool on = v < a->num_views;
        F.image[v] = on ? a->image[v] : nullptr; F.alpha[v] = on ? a->alpha[v] : nullptr;
        F.bound[v] = on ? a->bound[v] : nullptr; F.out[v] = on ? a->out[v] : nullptr;
        if (!on) continue;
        if (!F.image[v] || !F.out[v]) return invalid_arg(who, "null image or out of a view");
        if ((a->channels_out == 4) != (F.alpha[v] != nullptr)) return invalid_arg(who, "alpha is required with channels_out == 4 and only then");
        if (((uintptr_t)F.image[v] & 3u) || ((uintptr_t)F.alpha[v] & 3u)) return invalid_arg(who, "image or alpha not 4-byte aligned");
        // what the kernel's wide accesses rely on, and nothing more
        if (n % GROUP == 0 && ((uintptr_t)F.image[v] & 15u) == 0 && ((uintptr_t)F.alpha[v] & 15u) == 0 && ((uintptr_t)F.bound[v] & 3u) == 0)
            wide_in |= 1u << v;
        if (((uintptr_t)F.out[v] & 3u) == 0) wide_out |= 1u << v;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)a->num_views), block(256);
    if (a->channels_out == 3) {
        if (a->rounding == 0) hipLaunchKernelGGL((frames_to_u8_kernel<3, 0>), grid, block, 0, s, F, n, a->fill, wide_in, wide_out);
        else hipLaunchKernelGGL((frames_to_u8_kernel<3, 1>), grid, block, 0, s, F, n, a->fill, wide_in, wide_out);
    } else {
        if (a->rounding == 0) hipLaunchKernelGGL((frames_to_u8_kernel<4, 0>), grid, block, 0, s, F, n, a->fill, wide_in, wide_out);
        else hipLaunchKernelGGL((frames_to_u8_kernel<4, 1>), grid, block, 0, s, F, n, a->fill, wide_in, wide_out);
    }
    return launch_status(who);
}
