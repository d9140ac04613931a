// frame_bounds.hip -- what MOSS's dataset reader computes per (pose, camera) on the CPU (scene/dataset_readers.py:331-339, :428-439,
// :1008-1045), on the device: the posed SMPL vertices in the world, their padded axis-aligned box, and per camera the box's 2D bound
// mask with its bounding rectangle (include/moss_raster.h moss_smpl_vertices / moss_bound_mask; the formulas are restated there).
//
// moss_smpl_vertices, 3 launches:
//   posed          a grid over ranges of SMPL_VPB vertices (the form of smpl_frame.hip's offsets kernel: posedirs is the one large
//                  stream, 12 (J - 1) 9 V bytes, read once; one wave per 4 rows, lanes over the feature, a fixed butterfly).  Every
//                  workgroup recomputes the J rotations in LDS, forms f = rot[1:] - I, its rows of v_posed = v_template + shapedirs beta
//                  + posedirs f (kept in float64 in the workspace) and its share of J_regressor v_shaped.
//   skin           a grid over ranges of FB_SKIN_VPB vertices.  Every workgroup folds the regressor shares in a fixed order and walks
//                  the chain (one joint per step) -- cheaper than a launch that would hand 64 matrices over -- then four lanes per vertex
//                  form T_v = sum_j weights[v, j] A_j, R (T_v v_posed) + Th, write world_vertex and reduce the float32 values that were
//                  written to one min / max record per workgroup.  Workgroup 0 writes the posed joints.
//   bound          one wave folds the records in workgroup order and writes world_bound = fl32(min - pad), fl32(max + pad).
// moss_bound_mask, 2 launches for any number of cameras:
//   mask           a grid over (64 x 8 pixel tiles, cameras).  Every workgroup projects its camera's eight corners in float64 (eight
//                  lanes), then tests its pixels against the six faces in int64 and writes bound; one (min x, min y, max x, max y,
//                  count) record per workgroup.  Tile 0 of a camera writes its corners and flag.
//   rect           one workgroup per camera folds its records.
// moss_smpl_vertices_backward (g_poses, g_R, g_Th of a g_world_vertex), 4 launches; nothing is saved by the forward:
//   posed          the forward's kernel as it is: v_posed and the regressor shares.
//   skin adjoint   the skin kernel's grid and chain; one thread per vertex forms y_v, h_v = R^T g_v and g_vposed_v = T_v[:3,:3]^T h_v, then
//                  one thread per output walks the workgroup's vertices in index order: its partial sums of g_Th, g_R and g_A.
//   features       a grid over ranges of FB_FEAT_VPB vertices, threads over the pose features (the form of smpl_frame.hip's reduce
//                  kernel): sum_v sum_c posedirs[v, c, k] g_vposed[v, c], one partial vector per workgroup; posedirs is read once.
//   chain adjoint  one workgroup folds both sets of partials in a fixed order, walks the tree in reverse (smpl_frame.hip's walk on the
//                  float64 chain recomputed here) and forms the adjoint of Rodrigues, one joint per thread.
// Every sum is formed in float64 in a fixed order, nothing is atomic, every output element is written: bitwise reproducible.
// Nothing is allocated, nothing synchronises, nothing is cleared with a memset.  Every loop's trip count is fixed by the arguments.
#include "common.h"
#include "smpl_math.h"
#include "wave.h"
#include <limits.h>

namespace moss {

namespace {

constexpr int FB_BLOCK = 256;
constexpr int FB_SKIN_BLOCK = 1024;
constexpr int FB_SKIN_VPB = 256;          // vertices per workgroup of the skin kernel: four lanes each (three rows, one idle)
constexpr int FB_FEAT_VPB = 32;           // vertices per workgroup of the backward's feature kernel
constexpr int FB_TILE_W = 64, FB_TILE_H = 8;
constexpr int FB_ROWS = FB_TILE_H / (FB_BLOCK / 64);    // rows of a tile per wave
constexpr int FB_CLAMP = 1 << 20;

struct FbIn {
    int V, J, nb, sd_stride;
    const float* vt;
    const float* sd;
    const float* pd;
    const float* jr;
    const float* w;
    const float* poses;
    const float* shapes;
    const float* R;
    const float* Th;
};

// v_posed rows (float64) and regressor shares of vertices [SMPL_VPB b, SMPL_VPB (b + 1)); partials [workgroup][J][3]
__global__ void __launch_bounds__(FB_BLOCK)
frame_bounds_posed_kernel(FbIn a, double* __restrict__ vposed, double* __restrict__ partials)
{
    __shared__ float s_rot[SMPL_MAX_J * 9];
    __shared__ float s_f[SMPL_MAX_F + 1];
    __shared__ double s_vs[1][SMPL_VPB * 3];                  // the shaped template
    for (int j = threadIdx.x; j < a.J; j += FB_BLOCK) sf_rodrigues(a.poses + 3 * j, s_rot + 9 * j);
    __syncthreads();
    const int F = 9 * (a.J - 1);
    for (int k = threadIdx.x; k < F; k += FB_BLOCK) s_f[k] = s_rot[9 + k] - ((k % 9) % 4 == 0 ? 1.0f : 0.0f);
    const int v0 = blockIdx.x * SMPL_VPB;
    const int nv = min(SMPL_VPB, a.V - v0);
    const int nrows = nv * 3;
    if ((int)threadIdx.x < nrows) {
        const size_t row = (size_t)v0 * 3 + threadIdx.x;
        const float* sd = a.sd + row * a.sd_stride;
        double so = 0.0;
        for (int b = 0; b < a.nb; b++) so = fma((double)sd[b], (double)a.shapes[b], so);
        s_vs[0][threadIdx.x] = (double)a.vt[row] + so;
    }
    __syncthreads();
    smpl_regressor_shares<1, FB_BLOCK>(a.jr, a.V, a.J, v0, nv, s_vs, partials);
    if (F == 0) {                                             // (J = 1: no pose blend shapes, posedirs may be NULL; s_vs + 0.0 would lose a -0.0)
        if ((int)threadIdx.x < nrows) vposed[(size_t)v0 * 3 + threadIdx.x] = s_vs[0][threadIdx.x];
        return;
    }
    smpl_pose_blend_rows<FB_BLOCK>(a.pd, s_f, F, v0, nrows, [&](int r, double acc) { vposed[(size_t)v0 * 3 + r] = s_vs[0][r] + acc; });
}

// a workgroup of FB_SKIN_BLOCK threads: the rotations, the joints (the shares folded in a fixed order), the relative joints, the chain
// s_G (per joint: the rotation (9, row-major), then the translation (3)) and, unless s_A is null, rows 0..2 of A_j (3 x 4, row-major).
// The caller's next barrier publishes s_A.
__device__ __forceinline__ void fb_stage_chain(const FbIn& a, const SmplParents& par, int nparts, const double* __restrict__ partials,
                                               float* s_rot, double* s_slice, double (*s_jt)[SMPL_MAX_J * 3],
                                               double (*s_rel)[SMPL_MAX_J * 3], double* s_G, double* s_A)
{
    const int t = threadIdx.x;
    const int J = a.J;
    for (int j = t; j < J; j += FB_SKIN_BLOCK) sf_rodrigues(a.poses + 3 * j, s_rot + 9 * j);
    smpl_fold_shares<1, FB_SKIN_BLOCK>(J, nparts, partials, s_slice, s_jt);         // (nslice >= 5; its first barrier covers s_rot)
    smpl_relative_joints<1>(J, par, s_jt, s_rel);
    for (int j = 0; j < J; j++) {
        if (t < 12) smpl_chain_step(j, t, par, s_rot + 9 * j, s_rel[0] + 3 * j, s_G);
        __syncthreads();
    }
    if (!s_A) return;
    for (int o = t; o < J * 12; o += FB_SKIN_BLOCK) {
        const int j = o / 12;
        s_A[o] = smpl_A_entry(s_G + 12 * j, s_jt[0] + 3 * j, (o % 12) / 4, o % 4);
    }
}

// every workgroup: the joints (the shares folded in a fixed order), the chain, A; then its vertices and their min / max record
__global__ void __launch_bounds__(FB_SKIN_BLOCK)
frame_bounds_skin_kernel(FbIn a, SmplParents par, int nparts, const double* __restrict__ partials, const double* __restrict__ vposed,
                         float* __restrict__ world_vertex, float* __restrict__ joints, float* __restrict__ records)
{
    __shared__ float s_rot[SMPL_MAX_J * 9];
    __shared__ double s_slice[FB_SKIN_BLOCK];
    __shared__ double s_jt[1][SMPL_MAX_J * 3], s_rel[1][SMPL_MAX_J * 3];
    __shared__ double s_G[SMPL_MAX_J * 12];
    __shared__ double s_A[SMPL_MAX_J * 12];
    __shared__ double s_p[FB_SKIN_VPB * 3];
    __shared__ float s_mm[FB_SKIN_BLOCK / 64][6];
    const int t = threadIdx.x;
    const int J = a.J, nout = J * 3;
    fb_stage_chain(a, par, nparts, partials, s_rot, s_slice, s_jt, s_rel, s_G, s_A);
    if (joints && blockIdx.x == 0 && t < nout) joints[t] = (float)s_G[12 * (t / 3) + 9 + t % 3];
    __syncthreads();
    const int vl = t >> 2, r = t & 3;
    const int v = blockIdx.x * FB_SKIN_VPB + vl;
    const bool active = v < a.V && r < 3;
    if (active) {
        const float* w = a.w + (size_t)v * J;
        double T0 = 0.0, T1 = 0.0, T2 = 0.0, T3 = 0.0;
        for (int j = 0; j < J; j++) {
            const double wj = (double)w[j];
            const double* A = s_A + 12 * j + 4 * r;
            T0 = fma(wj, A[0], T0); T1 = fma(wj, A[1], T1); T2 = fma(wj, A[2], T2); T3 = fma(wj, A[3], T3);
        }
        const double* vp = vposed + (size_t)v * 3;
        s_p[3 * vl + r] = T0 * vp[0] + T1 * vp[1] + T2 * vp[2] + T3;
    }
    __syncthreads();
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (active) {
        const double* p = s_p + 3 * vl;
        const float* R = a.R + 3 * r;
        const float out = (float)((double)R[0] * p[0] + (double)R[1] * p[1] + (double)R[2] * p[2] + (double)a.Th[r]);
        world_vertex[(size_t)v * 3 + r] = out;
        lo = hi = out;
    }
#pragma unroll
    for (int d = 32; d >= 4; d >>= 1) {                       // (lanes of one component: the same lane & 3)
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    if ((t & 63) < 3) {
        s_mm[t >> 6][t & 63] = lo;
        s_mm[t >> 6][3 + (t & 63)] = hi;
    }
    __syncthreads();
    if (t < 6) {
        float m = s_mm[0][t];
        for (int wv = 1; wv < FB_SKIN_BLOCK / 64; wv++) m = t < 3 ? fminf(m, s_mm[wv][t]) : fmaxf(m, s_mm[wv][t]);
        records[(size_t)blockIdx.x * 6 + t] = m;
    }
}

// world_bound (2,3): the records in workgroup order, then - pad / + pad in float32
__global__ void __launch_bounds__(64)
frame_bounds_fold_kernel(int nrecords, const float* __restrict__ records, const float* __restrict__ pad, float* __restrict__ world_bound)
{
    const int t = threadIdx.x;
    if (t >= 6) return;
    float m = records[t];
    for (int b = 1; b < nrecords; b++) m = t < 3 ? fminf(m, records[(size_t)b * 6 + t]) : fmaxf(m, records[(size_t)b * 6 + t]);
    const float p = pad[0];
    world_bound[t] = t < 3 ? m - p : m + p;
}

// ---- moss_smpl_vertices_backward ---------------------------------------------------------------------------------------------------

// the skin kernel's grid: g_vposed rows of vertices [FB_SKIN_VPB b, FB_SKIN_VPB (b + 1)) and sums [workgroup][12 J + 12]: the workgroup's
// share of g_A (J x 3 x 4), then of g_R (9), then of g_Th (3), its vertices taken in index order
__global__ void __launch_bounds__(FB_SKIN_BLOCK)
frame_bounds_skin_backward_kernel(FbIn a, SmplParents par, int nparts, const double* __restrict__ partials, const double* __restrict__ vposed,
                                  const float* __restrict__ g_world, double* __restrict__ g_vposed, double* __restrict__ sums)
{
    __shared__ float s_rot[SMPL_MAX_J * 9];
    __shared__ double s_slice[FB_SKIN_BLOCK];
    __shared__ double s_jt[1][SMPL_MAX_J * 3], s_rel[1][SMPL_MAX_J * 3];
    __shared__ double s_G[SMPL_MAX_J * 12];
    __shared__ double s_A[SMPL_MAX_J * 12];
    __shared__ double s_vp[FB_SKIN_VPB * 3], s_y[FB_SKIN_VPB * 3], s_g[FB_SKIN_VPB * 3], s_h[FB_SKIN_VPB * 3];
    const int t = threadIdx.x;
    const int J = a.J;
    fb_stage_chain(a, par, nparts, partials, s_rot, s_slice, s_jt, s_rel, s_G, s_A);
    __syncthreads();
    const int v0 = blockIdx.x * FB_SKIN_VPB;
    const int nv = min(FB_SKIN_VPB, a.V - v0);
    if (t < nv) {
        const int v = v0 + t;
        const float* w = a.w + (size_t)v * J;
        double T[12];
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = 0.0;
#pragma unroll 4
        for (int j = 0; j < J; j++) {
            const double wj = (double)w[j];
            const double* A = s_A + 12 * j;
#pragma unroll
            for (int e = 0; e < 12; e++) T[e] = fma(wj, A[e], T[e]);
        }
        const double* vp = vposed + (size_t)v * 3;
        const double p0 = vp[0], p1 = vp[1], p2 = vp[2];
        const float* gw = g_world + (size_t)v * 3;
        const double g0 = (double)gw[0], g1 = (double)gw[1], g2 = (double)gw[2];
        double h[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            h[c] = (double)a.R[c] * g0 + (double)a.R[3 + c] * g1 + (double)a.R[6 + c] * g2;                     // R^T g
            s_y[3 * t + c] = T[4 * c] * p0 + T[4 * c + 1] * p1 + T[4 * c + 2] * p2 + T[4 * c + 3];
        }
        s_vp[3 * t] = p0; s_vp[3 * t + 1] = p1; s_vp[3 * t + 2] = p2;
        s_g[3 * t] = g0; s_g[3 * t + 1] = g1; s_g[3 * t + 2] = g2;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_h[3 * t + c] = h[c];
            g_vposed[(size_t)v * 3 + c] = T[c] * h[0] + T[4 + c] * h[1] + T[8 + c] * h[2];                      // T[:3,:3]^T h
        }
    }
    __syncthreads();
    const int nsum = 12 * J + 12;
    if (t >= nsum) return;
    double acc = 0.0;
    if (t < 12 * J) {                                          // g_A_j[r][c] = sum_v w[v, j] h_v[r] [v_posed_v, 1][c]
        const int j = t / 12, r = (t % 12) / 4, c = t % 4;
        const float* w = a.w + (size_t)v0 * J + j;
#pragma unroll 8
        for (int i = 0; i < nv; i++) {                        // (unrolled: eight weights in flight; the order of the sum is the loop's)
            const double wh = (double)w[(size_t)i * J] * s_h[3 * i + r];
            acc = c < 3 ? fma(wh, s_vp[3 * i + c], acc) : acc + wh;
        }
    } else if (t < 12 * J + 9) {                               // g_R[r][c] = sum_v g_v[r] y_v[c]
        const int r = (t - 12 * J) / 3, c = (t - 12 * J) % 3;
        for (int i = 0; i < nv; i++) acc = fma(s_g[3 * i + r], s_y[3 * i + c], acc);
    } else {                                                   // g_Th[r] = sum_v g_v[r]
        const int r = t - 12 * J - 9;
        for (int i = 0; i < nv; i++) acc += s_g[3 * i + r];
    }
    sums[(size_t)blockIdx.x * nsum + t] = acc;
}

// fpartials[workgroup][k] = sum over the workgroup's vertices, in index order, of sum_c posedirs[v, c, k] g_vposed[v, c]
__global__ void __launch_bounds__(FB_BLOCK)
frame_bounds_feature_backward_kernel(int V, int F, const float* __restrict__ pd, const double* __restrict__ g_vposed,
                                     double* __restrict__ fpartials)
{
    __shared__ double s_g[FB_FEAT_VPB * 3];
    const int t = threadIdx.x;
    const int v0 = blockIdx.x * FB_FEAT_VPB;
    const int n = min(FB_FEAT_VPB, V - v0);
    if (t < n * 3) s_g[t] = g_vposed[(size_t)v0 * 3 + t];
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int q = 0; q < n; q++) {
        const float* row = pd + (size_t)(v0 + q) * 3 * F;
        const double g0 = s_g[3 * q], g1 = s_g[3 * q + 1], g2 = s_g[3 * q + 2];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const int k = t + FB_BLOCK * s;
            if (k < F) acc[s] = fma((double)row[k], g0, fma((double)row[F + k], g1, fma((double)row[2 * F + k], g2, acc[s])));
        }
    }
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const int k = t + FB_BLOCK * s;
        if (k < F) fpartials[(size_t)blockIdx.x * F + k] = acc[s];
    }
}

// one workgroup: both sets of partials folded in a fixed order, g_R and g_Th written; then the adjoint of the chain as
// smpl_frame.hip's chain adjoint states it (gGR_j = gA_j[:3,:3] - gA_j[:3,3] joint_j^T, gGt_j = gA_j[:3,3]; j = J-1 .. 1:
// g_rot_j = GR_p^T gGR_j, gGR_p += gGR_j rot_j^T + gGt_j rel_j^T, gGt_p += gGt_j; g_rot_0 = gGR_0) on the chain recomputed here in
// float64, g_raw_j = g_rot_j + g_feat_j, and the adjoint of Rodrigues, one joint per thread
__global__ void __launch_bounds__(FB_SKIN_BLOCK)
frame_bounds_chain_backward_kernel(FbIn a, SmplParents par, int nparts, const double* __restrict__ partials, int nskin,
                                   const double* __restrict__ sums, int nfeat, const double* __restrict__ fpartials,
                                   float* __restrict__ g_poses, float* __restrict__ g_R, float* __restrict__ g_Th)
{
    __shared__ float s_rot[SMPL_MAX_J * 9];
    __shared__ double s_slice[FB_SKIN_BLOCK];
    __shared__ double s_jt[1][SMPL_MAX_J * 3], s_rel[1][SMPL_MAX_J * 3];
    __shared__ double s_G[SMPL_MAX_J * 12];
    __shared__ double s_gA[SMPL_MAX_J * 12];
    __shared__ double s_gGR[SMPL_MAX_J * 9], s_gGt[SMPL_MAX_J * 3], s_gR[SMPL_MAX_J * 9];
    const int t = threadIdx.x;
    const int J = a.J;
    fb_stage_chain(a, par, nparts, partials, s_rot, s_slice, s_jt, s_rel, s_G, nullptr);
    // g_feat as smpl_fold_shares folds the joints: the feature partials cut into nslice = FB_SKIN_BLOCK / F runs of workgroups, each
    // summed in order (here), then the runs in order (after the walk) -- a function of V and J only
    const int F = 9 * (J - 1);
    const int nslice = F ? FB_SKIN_BLOCK / F : 0;
    if (t < F * nslice) {
        const int k = t % F, sl = t / F;
        const int per = (nfeat + nslice - 1) / nslice;
        const int b1 = min(nfeat, (sl + 1) * per);
        double acc = 0.0;
#pragma unroll 8
        for (int b = sl * per; b < b1; b++) acc += fpartials[(size_t)b * F + k];
        s_slice[t] = acc;
    }
    const int nsum = 12 * J + 12;
    for (int o = t; o < nsum; o += FB_SKIN_BLOCK) {
        double acc = 0.0;
#pragma unroll 9
        for (int b = 0; b < nskin; b++) acc += sums[(size_t)b * nsum + o];
        if (o < 12 * J) s_gA[o] = acc;
        else if (o < 12 * J + 9) g_R[o - 12 * J] = (float)acc;
        else g_Th[o - 12 * J - 9] = (float)acc;
    }
    __syncthreads();
    const double* jt = s_jt[0];
    const double* rel = s_rel[0];
    for (int e = t; e < J * 12; e += FB_SKIN_BLOCK) {
        const int j = e / 12, q = e % 12;
        if (q < 9) {
            const int r = q / 3, c = q % 3;
            s_gGR[9 * j + q] = s_gA[12 * j + 4 * r + c] - s_gA[12 * j + 4 * r + 3] * jt[3 * j + c];
            s_gR[9 * j + q] = 0.0;
        } else {
            s_gGt[3 * j + q - 9] = s_gA[12 * j + 4 * (q - 9) + 3];
        }
    }
    __syncthreads();
    for (int j = J - 1; j >= 1; j--) {
        const int p = par.p[j];
        if (t < 9) {
            const int r = t / 3, c = t % 3;
            const double* g = s_gGR + 9 * j;
            const double* GRp = s_G + 12 * p;
            s_gR[9 * j + t] = GRp[r] * g[c] + GRp[3 + r] * g[3 + c] + GRp[6 + r] * g[6 + c];
            const float* Rj = s_rot + 9 * j;
            s_gGR[9 * p + t] += g[3 * r] * (double)Rj[3 * c] + g[3 * r + 1] * (double)Rj[3 * c + 1] + g[3 * r + 2] * (double)Rj[3 * c + 2]
                              + s_gGt[3 * j + r] * rel[3 * j + c];
        } else if (t < 12) {
            s_gGt[3 * p + t - 9] += s_gGt[3 * j + t - 9];
        }
        __syncthreads();
    }
    for (int k = t; k < F; k += FB_SKIN_BLOCK) {
        double acc = 0.0;
        for (int sl = 0; sl < nslice; sl++) acc += s_slice[sl * F + k];
        s_gR[9 + k] += acc;
    }
    if (t < 9) s_gR[t] = s_gGR[t];                            // (thread t wrote s_gGR[t] itself in the walk's last steps)
    __syncthreads();
    if (t >= J) return;
    double G[9];
#pragma unroll
    for (int e = 0; e < 9; e++) G[e] = s_gR[9 * t + e];
    smpl_rodrigues_adjoint(G, a.poses + 3 * t, g_poses + 3 * t);
}

// (min x, min y, max x, max y, count) of a workgroup from its threads' values; valid in thread 0
__device__ __forceinline__ void fb_block_record(int (*s_rec)[5], int& x0, int& y0, int& x1, int& y1, int& n)
{
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1); n = wave_sum(n);
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) { s_rec[wave][0] = x0; s_rec[wave][1] = y0; s_rec[wave][2] = x1; s_rec[wave][3] = y1; s_rec[wave][4] = n; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int wv = 1; wv < FB_BLOCK / 64; wv++) {
            x0 = min(x0, s_rec[wv][0]); y0 = min(y0, s_rec[wv][1]); x1 = max(x1, s_rec[wv][2]); y1 = max(y1, s_rec[wv][3]);
            n += s_rec[wv][4];
        }
}

// one corner of the box through project() (dataset_readers.py:1023-1032) in float64, every operation rounded on its own, and np.round;
// returns the flag bit
__device__ __forceinline__ int fb_project(const float* __restrict__ wb, const float* __restrict__ K, const float* __restrict__ RT, int i,
                                          int* xy)
{
#pragma clang fp contract(off)
    const double c0 = (double)wb[(i & 4) ? 3 : 0], c1 = (double)wb[(i & 2) ? 4 : 1], c2 = (double)wb[(i & 1) ? 5 : 2];
    double cam[3], uvw[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
        cam[r] = ((c0 * (double)RT[4 * r] + c1 * (double)RT[4 * r + 1]) + c2 * (double)RT[4 * r + 2]) + (double)RT[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 3; r++)
        uvw[r] = (cam[0] * (double)K[3 * r] + cam[1] * (double)K[3 * r + 1]) + cam[2] * (double)K[3 * r + 2];
    int flag = uvw[2] <= 0.0 ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        double q = rint(uvw[k] / uvw[2]);
        if (!(fabs(q) <= (double)FB_CLAMP)) flag = 1;
        if (!(q >= -(double)FB_CLAMP)) q = -(double)FB_CLAMP;      // (a NaN lands here)
        if (q > (double)FB_CLAMP) q = (double)FB_CLAMP;
        xy[k] = (int)q;
    }
    return flag;
}

__constant__ int8_t FB_FACES[6][4] = {{0, 1, 3, 2}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 3, 7, 5}};

// bound of tile blockIdx.x of camera blockIdx.y and the tile's record; tile 0 also writes the camera's corners and flag
__global__ void __launch_bounds__(FB_BLOCK)
frame_bounds_mask_kernel(int H, int W, int tiles_x, const float* __restrict__ world_bound, const float* __restrict__ Ks,
                         const float* __restrict__ RTs, uint8_t* __restrict__ bound, int32_t* __restrict__ corners,
                         int32_t* __restrict__ flags, int32_t* __restrict__ records)
{
    __shared__ int s_q[8][2];
    __shared__ int s_cflag[8];
    __shared__ int s_face[6][4];                             // per face: x0, x1, y0, y1 of its bounding box
    __shared__ int s_edge[24][5];                            // per face and edge k: q_k.x, q_k.y, dx, dy, m = max(|dx|, |dy|)
    __shared__ int s_rec[FB_BLOCK / 64][5];
    const int t = threadIdx.x;
    const int cam = blockIdx.y;
    if (t < 8) s_cflag[t] = fb_project(world_bound, Ks + (size_t)cam * 9, RTs + (size_t)cam * 12, t, s_q[t]);
    __syncthreads();
    int flag = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) flag |= s_cflag[i];
    if (t < 6) {
        int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int* q = s_q[FB_FACES[t][k]];
            x0 = min(x0, q[0]); x1 = max(x1, q[0]); y0 = min(y0, q[1]); y1 = max(y1, q[1]);
        }
        s_face[t][0] = x0; s_face[t][1] = x1; s_face[t][2] = y0; s_face[t][3] = y1;
    } else if (t >= 64 && t < 88) {                           // (corners within +-2^20: the differences fit an int)
        const int e = t - 64, f = e >> 2, k = e & 3;
        const int* q0 = s_q[FB_FACES[f][k]];
        const int* q1 = s_q[FB_FACES[f][(k + 1) & 3]];
        const int dx = q1[0] - q0[0], dy = q1[1] - q0[1];
        s_edge[e][0] = q0[0]; s_edge[e][1] = q0[1]; s_edge[e][2] = dx; s_edge[e][3] = dy; s_edge[e][4] = max(abs(dx), abs(dy));
    }
    if (blockIdx.x == 0) {
        if (t < 16) corners[(size_t)cam * 16 + t] = s_q[t / 2][t % 2];
        if (t == 0) flags[cam] = flag;
    }
    __syncthreads();
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x = tx * FB_TILE_W + (t & 63);
    const int ybase = ty * FB_TILE_H + (t >> 6) * FB_ROWS;
    int rx0 = INT_MAX, ry0 = INT_MAX, rx1 = -1, ry1 = -1, n = 0;
    if (x < W) {
        uint8_t* out = bound + (size_t)cam * H * W;
        for (int i = 0; i < FB_ROWS; i++) {
            const int y = ybase + i;
            if (y >= H) break;
            bool in = flag != 0;
            for (int f = 0; f < 6 && !in; f++) {
                if (x < s_face[f][0] || x > s_face[f][1] || y < s_face[f][2] || y > s_face[f][3]) continue;
                bool ge = true, le = true, edge = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int* e = s_edge[4 * f + k];
                    const int64_t dx = e[2], dy = e[3];
                    const int64_t cr = dx * ((int64_t)y - e[1]) - dy * ((int64_t)x - e[0]);
                    ge &= cr >= 0;
                    le &= cr <= 0;
                    const int64_t ex = (int64_t)x - e[0], ey = (int64_t)y - e[1];  // inside the edge's box: between q_k and q_k + (dx, dy) on both axes
                    const bool inbox = (e[2] >= 0 ? ex >= 0 && ex <= e[2] : ex <= 0 && ex >= e[2])
                                    && (e[3] >= 0 ? ey >= 0 && ey <= e[3] : ey <= 0 && ey >= e[3]);
                    const int64_t c2 = 2 * cr;
                    edge |= inbox && (c2 < 0 ? -c2 : c2) <= (int64_t)e[4];
                }
                in = ge || le || edge;
            }
            out[(size_t)y * W + x] = in ? 1 : 0;
            if (in) { rx0 = min(rx0, x); rx1 = max(rx1, x); ry0 = min(ry0, y); ry1 = max(ry1, y); n++; }
        }
    }
    fb_block_record(s_rec, rx0, ry0, rx1, ry1, n);
    if (t == 0) {
        int32_t* rec = records + ((size_t)cam * gridDim.x + blockIdx.x) * 5;
        rec[0] = rx0; rec[1] = ry0; rec[2] = rx1; rec[3] = ry1; rec[4] = n;
    }
}

// rect of camera blockIdx.x: its tiles' records folded (min, max and an integer sum: any order gives the same bits)
__global__ void __launch_bounds__(FB_BLOCK)
frame_bounds_rect_kernel(int ntiles, const int32_t* __restrict__ records, int32_t* __restrict__ rect)
{
    __shared__ int s_rec[FB_BLOCK / 64][5];
    const int cam = blockIdx.x;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1, n = 0;
    for (int b = threadIdx.x; b < ntiles; b += FB_BLOCK) {
        const int32_t* rec = records + ((size_t)cam * ntiles + b) * 5;
        x0 = min(x0, rec[0]); y0 = min(y0, rec[1]); x1 = max(x1, rec[2]); y1 = max(y1, rec[3]); n += rec[4];
    }
    fb_block_record(s_rec, x0, y0, x1, y1, n);
    if (threadIdx.x == 0) {
        int32_t* r = rect + (size_t)cam * 5;
        const bool any = n > 0;
        r[0] = any ? x0 : 0; r[1] = any ? y0 : 0; r[2] = any ? x1 - x0 + 1 : 0; r[3] = any ? y1 - y0 + 1 : 0; r[4] = n;
    }
}

size_t fb_vertices_bytes(int V, int J)
{
    const size_t nparts = ((size_t)V + SMPL_VPB - 1) / SMPL_VPB, nskin = ((size_t)V + FB_SKIN_VPB - 1) / FB_SKIN_VPB;
    return align_up((size_t)V * 3 * sizeof(double)) + align_up(nparts * (size_t)J * 3 * sizeof(double)) + align_up(nskin * 6 * sizeof(float));
}

struct FbBackwardCounts { size_t nparts, nskin, nfeat, nsum, F; };

FbBackwardCounts fb_backward_counts(int V, int J)
{
    const size_t F = 9 * (size_t)(J - 1);
    return {((size_t)V + SMPL_VPB - 1) / SMPL_VPB, ((size_t)V + FB_SKIN_VPB - 1) / FB_SKIN_VPB,
            F ? ((size_t)V + FB_FEAT_VPB - 1) / FB_FEAT_VPB : 0, 12 * (size_t)J + 12, F};
}

// v_posed, the regressor shares, g_vposed, the skin adjoint's sums, the feature partials
size_t fb_backward_bytes(int V, int J)
{
    const FbBackwardCounts n = fb_backward_counts(V, J);
    return 2 * align_up((size_t)V * 3 * sizeof(double)) + align_up(n.nparts * (size_t)J * 3 * sizeof(double))
         + align_up(n.nskin * n.nsum * sizeof(double)) + align_up(n.nfeat * n.F * sizeof(double));
}

size_t fb_tiles(int H, int W) { return (((size_t)W + FB_TILE_W - 1) / FB_TILE_W) * (((size_t)H + FB_TILE_H - 1) / FB_TILE_H); }

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_smpl_vertices_workspace_bytes(int V, int J)
{
    if (V <= 0 || J < 1 || J > SMPL_MAX_J) return 0;
    return fb_vertices_bytes(V, J);
}

extern "C" int moss_smpl_vertices(const moss_smpl_vertices_args* a, void* stream)
{
    const char* who = "moss_smpl_vertices";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (a->J < 1 || a->J > SMPL_MAX_J) return invalid_arg(who, "J must be 1..64");
    if (a->num_betas < 0 || a->num_betas > a->shapedirs_stride) return invalid_arg(who, "num_betas must be 0..shapedirs_stride");
    if (!a->v_template || !a->shapedirs || !a->J_regressor || !a->weights || (a->J > 1 && !a->posedirs))
        return invalid_arg(who, "null body-model array (v_template, shapedirs, posedirs, J_regressor, weights)");
    if (!a->poses || !a->R || !a->Th || !a->pad || (a->num_betas > 0 && !a->shapes))
        return invalid_arg(who, "null frame input (poses, shapes, R, Th, pad)");
    if (!a->world_vertex || !a->world_bound) return invalid_arg(who, "null output (world_vertex, world_bound)");
    if (int rc = smpl_check_parents(who, a->J, a->parents)) return rc;
    if (!a->workspace || a->workspace_bytes < fb_vertices_bytes(a->V, a->J))
        return invalid_arg(who, "needs moss_smpl_vertices_workspace_bytes(V, J) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    const FbIn in{a->V, a->J, a->num_betas, a->shapedirs_stride, a->v_template, a->shapedirs, a->posedirs, a->J_regressor, a->weights,
                  a->poses, a->shapes, a->R, a->Th};
    const SmplParents par = smpl_parents(a);
    const int nparts = (a->V + SMPL_VPB - 1) / SMPL_VPB, nskin = (a->V + FB_SKIN_VPB - 1) / FB_SKIN_VPB;
    char* p = a->workspace;
    double* vposed = carve<double>(p, (size_t)a->V * 3);
    double* partials = carve<double>(p, (size_t)nparts * a->J * 3);
    float* records = carve<float>(p, (size_t)nskin * 6);
    hipLaunchKernelGGL(frame_bounds_posed_kernel, dim3(nparts), dim3(FB_BLOCK), 0, s, in, vposed, partials);
    hipLaunchKernelGGL(frame_bounds_skin_kernel, dim3(nskin), dim3(FB_SKIN_BLOCK), 0, s, in, par, nparts, (const double*)partials,
                       (const double*)vposed, a->world_vertex, a->joints, records);
    hipLaunchKernelGGL(frame_bounds_fold_kernel, dim3(1), dim3(64), 0, s, nskin, (const float*)records, a->pad, a->world_bound);
    return launch_status(who);
}

extern "C" size_t moss_smpl_vertices_backward_workspace_bytes(int V, int J)
{
    if (V <= 0 || J < 1 || J > SMPL_MAX_J) return 0;
    return fb_backward_bytes(V, J);
}

extern "C" int moss_smpl_vertices_backward(const moss_smpl_vertices_backward_args* a, void* stream)
{
    const char* who = "moss_smpl_vertices_backward";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (a->J < 1 || a->J > SMPL_MAX_J) return invalid_arg(who, "J must be 1..64");
    if (a->num_betas < 0 || a->num_betas > a->shapedirs_stride) return invalid_arg(who, "num_betas must be 0..shapedirs_stride");
    if (!a->v_template || !a->shapedirs || !a->J_regressor || !a->weights || (a->J > 1 && !a->posedirs))
        return invalid_arg(who, "null body-model array (v_template, shapedirs, posedirs, J_regressor, weights)");
    if (!a->poses || !a->R || !a->Th || (a->num_betas > 0 && !a->shapes)) return invalid_arg(who, "null frame input (poses, shapes, R, Th)");
    if (!a->g_world_vertex) return invalid_arg(who, "null g_world_vertex");
    if (!a->g_poses || !a->g_R || !a->g_Th) return invalid_arg(who, "null output (g_poses, g_R, g_Th)");
    if (int rc = smpl_check_parents(who, a->J, a->parents)) return rc;
    if (!a->workspace || a->workspace_bytes < fb_backward_bytes(a->V, a->J))
        return invalid_arg(who, "needs moss_smpl_vertices_backward_workspace_bytes(V, J) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    const FbIn in{a->V, a->J, a->num_betas, a->shapedirs_stride, a->v_template, a->shapedirs, a->posedirs, a->J_regressor, a->weights,
                  a->poses, a->shapes, a->R, a->Th};
    const SmplParents par = smpl_parents(a);
    const FbBackwardCounts n = fb_backward_counts(a->V, a->J);
    char* p = a->workspace;
    double* vposed = carve<double>(p, (size_t)a->V * 3);
    double* partials = carve<double>(p, n.nparts * a->J * 3);
    double* g_vposed = carve<double>(p, (size_t)a->V * 3);
    double* sums = carve<double>(p, n.nskin * n.nsum);
    double* fpartials = carve<double>(p, n.nfeat * n.F);
    hipLaunchKernelGGL(frame_bounds_posed_kernel, dim3((unsigned)n.nparts), dim3(FB_BLOCK), 0, s, in, vposed, partials);
    hipLaunchKernelGGL(frame_bounds_skin_backward_kernel, dim3((unsigned)n.nskin), dim3(FB_SKIN_BLOCK), 0, s, in, par, (int)n.nparts,
                       (const double*)partials, (const double*)vposed, a->g_world_vertex, g_vposed, sums);
    if (n.nfeat)
        hipLaunchKernelGGL(frame_bounds_feature_backward_kernel, dim3((unsigned)n.nfeat), dim3(FB_BLOCK), 0, s, a->V, (int)n.F, a->posedirs,
                           (const double*)g_vposed, fpartials);
    hipLaunchKernelGGL(frame_bounds_chain_backward_kernel, dim3(1), dim3(FB_SKIN_BLOCK), 0, s, in, par, (int)n.nparts,
                       (const double*)partials, (int)n.nskin, (const double*)sums, (int)n.nfeat, (const double*)fpartials, a->g_poses,
                       a->g_R, a->g_Th);
    return launch_status(who);
}

extern "C" size_t moss_bound_mask_workspace_bytes(int C, int H, int W)
{
    if (C <= 0 || C > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return 0;
    return align_up((size_t)C * fb_tiles(H, W) * 5 * sizeof(int32_t));
}

extern "C" int moss_bound_mask(const moss_bound_mask_args* a, void* stream)
{
    const char* who = "moss_bound_mask";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->C < 1 || a->C > 65535) return invalid_arg(who, "C must be 1..65535");
    if (a->H < 1 || a->W < 1 || (int64_t)a->H * a->W > INT32_MAX) return invalid_arg(who, "H and W must be >= 1 with H * W < 2^31");
    if (!a->world_bound || !a->K || !a->RT) return invalid_arg(who, "null input (world_bound, K, RT)");
    if (!a->bound || !a->rect || !a->corners || !a->flags) return invalid_arg(who, "null output (bound, rect, corners, flags)");
    const size_t ntiles = fb_tiles(a->H, a->W);
    if (!a->workspace || a->workspace_bytes < align_up((size_t)a->C * ntiles * 5 * sizeof(int32_t)))
        return invalid_arg(who, "needs moss_bound_mask_workspace_bytes(C, H, W) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    int32_t* records = reinterpret_cast<int32_t*>(a->workspace);
    const int tiles_x = (a->W + FB_TILE_W - 1) / FB_TILE_W;
    hipLaunchKernelGGL(frame_bounds_mask_kernel, dim3((unsigned)ntiles, a->C), dim3(FB_BLOCK), 0, s, a->H, a->W, tiles_x, a->world_bound,
                       a->K, a->RT, a->bound, a->corners, a->flags, records);
    hipLaunchKernelGGL(frame_bounds_rect_kernel, dim3(a->C), dim3(FB_BLOCK), 0, s, (int)ntiles, (const int32_t*)records, a->rect);
    return launch_status(who);
}
