// smpl_frame.hip -- the per-frame, per-subject part of MOSS's coarse_deform_c2source (include/moss_raster.h moss_smpl_frame_forward /
// moss_smpl_frame_backward; the formulas are restated there): Rodrigues of the big pose and of the frame, the regressed joints of both
// shapes, both kinematic chains, the per-vertex offset table D and its gather at the Gaussians' vertices.
//
// forward, 2 launches:
//   offsets        a grid over ranges of SMPL_VPB vertices.  Every workgroup recomputes the 2 J rotations in LDS (48 sincos: cheaper than
//                  a launch that would hand them over), forms f = rot_obs[1:] - rot_big[1:], its rows of D = shapedirs beta_obs + posedirs f
//                  (one wave per 4 rows, lanes over the feature, a fixed butterfly) and its share of J_regressor (v_template +
//                  shapedirs beta) for both shapes, which goes to the workspace.
//   chain + gather workgroup 0 folds those shares in a fixed order, walks both chains (one joint per step: parent[j] < j is all that is
//                  known of the tree) and writes A_big, A_obs, rot_mats and what the backward needs; every other workgroup gathers
//                  d = D[vert_ids] meanwhile.
// backward, 3 launches (the "direct form": g_D (V,3) is never formed):
//   reduce         a grid over ranges of SF_GPW Gaussians, threads over the 9 (J - 1) pose features: the workgroup walks its Gaussians in
//                  index order and accumulates sum_c posedirs[ids[i], c, k] g_d[i, c]; one partial vector per workgroup.  Traffic is
//                  P rows of 12 (J - 1) 9 bytes from a table that lives in the caches; ids that coincide cost nothing extra.
//   fold           one wave per feature adds the partials in workgroup order (as lbs.hip's lbs_fold_kernel; wave.h's butterfly).
//   chain adjoint  one workgroup: g_A_obs through the chain as a reverse walk of the tree, + the folded features, then
//                  g_correct_Rs = rot_raw[1:]^T g_rot[1:].
// backward to the pose (moss_smpl_frame_backward_pose), the same 3 launches: the chain adjoint also keeps the root's g_rot_0 = gGR_0 and
//                  then, one joint per thread, forms g_raw_j = (g_rot_j + g_feat_j) correct_Rs[j-1]^T and the adjoint of Rodrigues.
// Every sum is formed in float64 in a fixed order, nothing is atomic, every output element is written: bitwise reproducible.
// Nothing is allocated, nothing synchronises, nothing is cleared with a memset.
#include "common.h"
#include "smpl_math.h"
#include "wave.h"

namespace moss {

namespace {

constexpr int SF_BLOCK = 256;
constexpr int SF_CHAIN_BLOCK = 1024;    // the chain / gather kernel: 1024 Gaussians per gathering workgroup
constexpr int SF_GPW = 64;              // Gaussians per workgroup of the backward reduction
constexpr int SF_FOLD_WAVES = 4;
constexpr int SF_SAVED_PER_J = MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT;   // rot_raw 9, rot 9, chain rotation 9, relative joint 3, joint 3

struct SfIn {
    int P, V, J, nb_big, nb, sd_stride;
    const float* vt;
    const float* sd;
    const float* pd;
    const float* jr;
    const float* poses_big;
    const float* shapes_big;
    const float* poses;
    const float* shapes;
    const float* cR;
    const int64_t* ids;
};

// s_big: the big pose's rotations; s_raw: the frame's; s_rot: the frame's with rot[1:] = raw[1:] correct_Rs (J x 9 floats each)
__device__ __forceinline__ void sf_stage_rotations(const SfIn& a, float* s_big, float* s_raw, float* s_rot)
{
    for (int t = threadIdx.x; t < 2 * a.J; t += blockDim.x) {
        const int j = t < a.J ? t : t - a.J;
        sf_rodrigues((t < a.J ? a.poses_big : a.poses) + 3 * j, (t < a.J ? s_big : s_raw) + 9 * j);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < a.J * 9; e += blockDim.x) {
        float v = s_raw[e];
        if (a.cR && e >= 9) {
            const int j = e / 9, r = (e % 9) / 3, c = e % 3;
            const float* m = a.cR + (j - 1) * 9;
            const float* row = s_raw + 9 * j + 3 * r;
            v = row[0] * m[c] + row[1] * m[3 + c] + row[2] * m[6 + c];
        }
        s_rot[e] = v;
    }
    __syncthreads();
}

// D rows and regressor shares of vertices [SMPL_VPB b, SMPL_VPB (b + 1)); partials [workgroup][J][2 shapes][3]
__global__ void __launch_bounds__(SF_BLOCK)
smpl_frame_offsets_kernel(SfIn a, float* __restrict__ D, double* __restrict__ partials)
{
    __shared__ float s_big[SMPL_MAX_J * 9], s_raw[SMPL_MAX_J * 9], s_rot[SMPL_MAX_J * 9];
    __shared__ float s_f[SMPL_MAX_F + 1];
    __shared__ double s_vs[2][SMPL_VPB * 3];                  // the shaped template of the big pose's / the frame's betas
    __shared__ double s_so[SMPL_VPB * 3];                     // shapedirs beta_obs
    sf_stage_rotations(a, s_big, s_raw, s_rot);
    const int F = 9 * (a.J - 1);
    for (int k = threadIdx.x; k < F; k += SF_BLOCK) s_f[k] = s_rot[9 + k] - s_big[9 + k];
    const int v0 = blockIdx.x * SMPL_VPB;
    const int nv = min(SMPL_VPB, a.V - v0);
    const int nrows = nv * 3;
    if ((int)threadIdx.x < nrows) {
        const size_t row = (size_t)v0 * 3 + threadIdx.x;
        const float* sd = a.sd + row * a.sd_stride;
        double so_big = 0.0, so = 0.0;
        for (int b = 0; b < a.nb_big; b++) so_big = fma((double)sd[b], (double)a.shapes_big[b], so_big);
        for (int b = 0; b < a.nb; b++) so = fma((double)sd[b], (double)a.shapes[b], so);
        const double base = (double)a.vt[row];
        s_vs[0][threadIdx.x] = base + so_big;
        s_vs[1][threadIdx.x] = base + so;
        s_so[threadIdx.x] = so;
    }
    __syncthreads();
    smpl_regressor_shares<2, SF_BLOCK>(a.jr, a.V, a.J, v0, nv, s_vs, partials);
    smpl_pose_blend_rows<SF_BLOCK>(a.pd, s_f, F, v0, nrows,
                                   [&](int r, double acc) { D[(size_t)v0 * 3 + r] = (float)(s_so[r] + acc); });
}

// workgroup 0: the joints (the shares folded in a fixed order), both chains, A_big, A_obs, rot_mats, saved; the others: d = D[ids]
__global__ void __launch_bounds__(SF_CHAIN_BLOCK)
smpl_frame_chain_gather_kernel(SfIn a, SmplParents par, int nparts, const double* __restrict__ partials, const float* __restrict__ D,
                               float* __restrict__ A_big, float* __restrict__ A_obs, float* __restrict__ d, float* __restrict__ rot_out,
                               float* __restrict__ saved)
{
    const int t = threadIdx.x;
    if (blockIdx.x > 0) {
        const int i = (blockIdx.x - 1) * SF_CHAIN_BLOCK + t;
        if (i >= a.P) return;
        const int64_t v = a.ids[i];
        const bool ok = v >= 0 && v < a.V;                     // an id outside [0, V) is never dereferenced: a NaN row
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int c = 0; c < 3; c++) d[(size_t)i * 3 + c] = ok ? D[(size_t)v * 3 + c] : nan;
        return;
    }
    __shared__ float s_big[SMPL_MAX_J * 9], s_raw[SMPL_MAX_J * 9], s_rot[SMPL_MAX_J * 9];
    __shared__ double s_slice[SF_CHAIN_BLOCK];
    __shared__ double s_jt[2][SMPL_MAX_J * 3], s_rel[2][SMPL_MAX_J * 3];
    __shared__ double s_G[2][SMPL_MAX_J * 12];                 // per joint: the chain's rotation (9, row-major), then its translation (3)
    sf_stage_rotations(a, s_big, s_raw, s_rot);
    const int J = a.J;
    smpl_fold_shares<2, SF_CHAIN_BLOCK>(J, nparts, partials, s_slice, s_jt);        // (nslice >= 2)
    smpl_relative_joints<2>(J, par, s_jt, s_rel);
    for (int j = 0; j < J; j++) {
        if (t < 24) {
            const int s = t / 12;
            smpl_chain_step(j, t % 12, par, (s ? s_rot : s_big) + 9 * j, s_rel[s] + 3 * j, s_G[s]);
        }
        __syncthreads();
    }
    for (int o = t; o < 2 * J * 16; o += SF_CHAIN_BLOCK) {
        const int s = o / (J * 16), e = o % (J * 16), j = e / 16, r = (e % 16) / 4, c = e % 4;
        const double v = r == 3 ? (c == 3 ? 1.0 : 0.0) : smpl_A_entry(s_G[s] + 12 * j, s_jt[s] + 3 * j, r, c);
        (s ? A_obs : A_big)[e] = (float)v;
    }
    for (int e = t; e < J * 9; e += SF_CHAIN_BLOCK) {
        rot_out[e] = s_rot[e];
        if (saved) {
            saved[e] = s_raw[e];
            saved[9 * J + e] = s_rot[e];
            saved[18 * J + e] = (float)s_G[1][12 * (e / 9) + e % 9];
        }
    }
    if (saved && t < J * 3) {
        saved[27 * J + t] = (float)s_rel[1][t];
        saved[30 * J + t] = (float)s_jt[1][t];
    }
}

// partials[workgroup][k] = sum over the workgroup's Gaussians, in index order, of sum_c posedirs[ids[i], c, k] g_d[i, c]
__global__ void __launch_bounds__(SF_BLOCK)
smpl_frame_reduce_kernel(int P, int V, int F, const int64_t* __restrict__ ids, const float* __restrict__ pd,
                         const float* __restrict__ g_d, double* __restrict__ partials)
{
    __shared__ int s_v[SF_GPW];
    __shared__ float s_g[SF_GPW * 3];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * SF_GPW;
    const int n = min(SF_GPW, P - i0);
    if (t < SF_GPW) {
        const int64_t v = t < n ? ids[i0 + t] : -1;
        const bool ok = v >= 0 && v < V;                       // an out-of-range id adds nothing (its g_d row is NaN by lbs_deform's contract)
        s_v[t] = ok ? (int)v : 0;
#pragma unroll
        for (int c = 0; c < 3; c++) s_g[3 * t + c] = ok ? g_d[(size_t)(i0 + t) * 3 + c] : 0.0f;
    }
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int q = 0; q < n; q++) {
        const float* row = pd + (size_t)s_v[q] * 3 * F;
        const double g0 = (double)s_g[3 * q], g1 = (double)s_g[3 * q + 1], g2 = (double)s_g[3 * q + 2];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const int k = t + SF_BLOCK * s;
            if (k < F) acc[s] = fma((double)row[k], g0, fma((double)row[F + k], g1, fma((double)row[2 * F + k], g2, acc[s])));
        }
    }
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const int k = t + SF_BLOCK * s;
        if (k < F) partials[(size_t)blockIdx.x * F + k] = acc[s];
    }
}

// g_feat[k]: one wave per feature, the partials in workgroup order (lane l takes l, l + 64, ...), then a fixed butterfly
__global__ void __launch_bounds__(64 * SF_FOLD_WAVES)
smpl_frame_fold_kernel(int F, int nblocks, const double* __restrict__ partials, double* __restrict__ g_feat)
{
    const int k = blockIdx.x * SF_FOLD_WAVES + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (k >= F) return;
    double acc = 0.0;
    for (int b = lane; b < nblocks; b += 64) acc += partials[(size_t)b * F + k];
    acc = wave_sum(acc);
    if (lane == 0) g_feat[k] = acc;
}

// the adjoint of the frame's chain and of rot[1:] = raw[1:] correct_Rs.  With G_j = G_p local_j (p = parent[j]) and
// A_j = [GR_j | Gt_j - GR_j joint_j]:  gGR_j = gA_j[:3,:3] - gA_j[:3,3] joint_j^T, gGt_j = gA_j[:3,3]; walking j = J-1 .. 1:
// g_rot_j = GR_p^T gGR_j, gGR_p += gGR_j rot_j^T + gGt_j rel_j^T, gGt_p += gGt_j.
//
// POSE (moss_smpl_frame_backward_pose; the other instantiation never reads poses, cR, g_poses): the root keeps g_rot_0 = gGR_0 (G_0.R = rot_0), and joint j (one per thread) forms
// g_raw_j = g_rot_j cR_j^T (cR_0 = I; cR = NULL: all I) and the adjoint of Rodrigues (smpl_math.h smpl_rodrigues_adjoint).
template <bool POSE>
__global__ void __launch_bounds__(SF_BLOCK)
smpl_frame_chain_backward_kernel(int J, SmplParents par, const float* __restrict__ saved, const float* __restrict__ gA,
                                 const double* __restrict__ g_feat, float* __restrict__ g_cR, const float* __restrict__ poses,
                                 const float* __restrict__ cR, float* __restrict__ g_poses)
{
    __shared__ float s_sv[SF_SAVED_PER_J * SMPL_MAX_J];
    __shared__ double s_gGR[SMPL_MAX_J * 9], s_gGt[SMPL_MAX_J * 3], s_gR[SMPL_MAX_J * 9];
    const int t = threadIdx.x;
    for (int e = t; e < SF_SAVED_PER_J * J; e += SF_BLOCK) s_sv[e] = saved[e];
    __syncthreads();
    const float* raw = s_sv;
    const float* rot = s_sv + 9 * J;
    const float* GR = s_sv + 18 * J;
    const float* rel = s_sv + 27 * J;
    const float* jt = s_sv + 30 * J;
    for (int e = t; e < J * 12; e += SF_BLOCK) {
        const int j = e / 12, q = e % 12;
        if (q < 9) {
            const int r = q / 3, c = q % 3;
            s_gGR[9 * j + q] = gA ? (double)gA[j * 16 + r * 4 + c] - (double)gA[j * 16 + r * 4 + 3] * (double)jt[3 * j + c] : 0.0;
            s_gR[9 * j + q] = 0.0;
        } else {
            s_gGt[3 * j + q - 9] = gA ? (double)gA[j * 16 + (q - 9) * 4 + 3] : 0.0;
        }
    }
    __syncthreads();
    if (gA) {                                                  // (uniform: without g_A_obs the chain carries nothing)
        for (int j = J - 1; j >= 1; j--) {
            const int p = par.p[j];
            if (t < 9) {
                const int r = t / 3, c = t % 3;
                const double* g = s_gGR + 9 * j;
                s_gR[9 * j + t] = (double)GR[9 * p + r] * g[c] + (double)GR[9 * p + 3 + r] * g[3 + c] + (double)GR[9 * p + 6 + r] * g[6 + c];
                const float* Rj = rot + 9 * j;
                s_gGR[9 * p + t] += g[3 * r] * (double)Rj[3 * c] + g[3 * r + 1] * (double)Rj[3 * c + 1] + g[3 * r + 2] * (double)Rj[3 * c + 2]
                                  + s_gGt[3 * j + r] * (double)rel[3 * j + c];
            } else if (t < 12) {
                s_gGt[3 * p + t - 9] += s_gGt[3 * j + t - 9];
            }
            __syncthreads();
        }
    }
    const int F = 9 * (J - 1);
    if (g_feat)
        for (int k = t; k < F; k += SF_BLOCK) s_gR[9 + k] += g_feat[k];
    if (POSE && t < 9) s_gR[t] = s_gGR[t];                   // (thread t wrote s_gGR[t] itself in the walk's last steps)
    __syncthreads();
    if (g_cR)
        for (int k = t; k < F; k += SF_BLOCK) {
            const int j = 1 + k / 9, r = (k % 9) / 3, c = k % 3;
            const float* m = raw + 9 * j;
            const double* g = s_gR + 9 * j;
            g_cR[k] = (float)((double)m[r] * g[c] + (double)m[3 + r] * g[3 + c] + (double)m[6 + r] * g[6 + c]);
        }
    if (!POSE || t >= J) return;
    const int j = t;
    double G[9];
    {
        const double* g = s_gR + 9 * j;
        if (cR && j >= 1) {
            const float* m = cR + 9 * (j - 1);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++)                          // g_raw = g_rot cR^T
                    G[3 * r + c] = g[3 * r] * (double)m[3 * c] + g[3 * r + 1] * (double)m[3 * c + 1] + g[3 * r + 2] * (double)m[3 * c + 2];
        } else {
#pragma unroll
            for (int e = 0; e < 9; e++) G[e] = g[e];
        }
    }
    smpl_rodrigues_adjoint(G, poses + 3 * j, g_poses + 3 * j);
}

size_t sf_forward_bytes(int V, int J)
{
    const size_t nparts = ((size_t)V + SMPL_VPB - 1) / SMPL_VPB;
    return align_up((size_t)V * 3 * sizeof(float)) + align_up(nparts * (size_t)J * 6 * sizeof(double));
}

size_t sf_backward_bytes(int P, int J)
{
    const size_t nblocks = ((size_t)P + SF_GPW - 1) / SF_GPW, F = 9 * (size_t)(J - 1);
    return align_up(nblocks * F * sizeof(double)) + align_up(F * sizeof(double));
}

// both backward entries: the checks, reduce -> fold (with g_d and Gaussians to read), the chain adjoint.  POSE: the block also has
// poses, correct_Rs and g_poses, g_correct_Rs is optional, and J = 1 still has the root's pose to differentiate
template <bool POSE, typename A>
int sf_backward_impl(const char* who, const A* a, void* stream)
{
    if (!a) return invalid_arg(who, "null argument block");
    if (a->P < 0) return invalid_arg(who, "P must be >= 0");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (a->J < 1 || a->J > SMPL_MAX_J) return invalid_arg(who, "J must be 1..64");
    const float* poses = nullptr;
    const float* cR = nullptr;
    float* g_poses = nullptr;
    if constexpr (POSE) {
        if (!a->g_poses) return invalid_arg(who, "null g_poses");
        if (!a->saved || !a->poses) return invalid_arg(who, "null saved or poses");
        poses = a->poses; cR = a->correct_Rs; g_poses = a->g_poses;
    } else {
        if (a->J == 1) return 0;                               // no joint has a correct_Rs: nothing to write
        if (!a->saved || !a->g_correct_Rs) return invalid_arg(who, "null saved or g_correct_Rs");
    }
    if (int rc = smpl_check_parents(who, a->J, a->parents)) return rc;
    const bool reduce = a->g_d && a->P > 0 && a->J > 1;
    if (reduce && (!a->vert_ids || !a->posedirs)) return invalid_arg(who, "g_d needs vert_ids and posedirs");
    if (reduce && (!a->workspace || a->workspace_bytes < sf_backward_bytes(a->P, a->J)))
        return invalid_arg(who, "g_d needs moss_smpl_frame_workspace_bytes(P, V, J) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    const int F = 9 * (a->J - 1);
    double* g_feat = nullptr;
    if (reduce) {
        const int nblocks = (a->P + SF_GPW - 1) / SF_GPW;
        double* partials = reinterpret_cast<double*>(a->workspace);
        g_feat = reinterpret_cast<double*>(a->workspace + align_up((size_t)nblocks * F * sizeof(double)));
        hipLaunchKernelGGL(smpl_frame_reduce_kernel, dim3(nblocks), dim3(SF_BLOCK), 0, s, a->P, a->V, F, a->vert_ids, a->posedirs, a->g_d,
                           partials);
        hipLaunchKernelGGL(smpl_frame_fold_kernel, dim3((F + SF_FOLD_WAVES - 1) / SF_FOLD_WAVES), dim3(64 * SF_FOLD_WAVES), 0, s, F,
                           nblocks, (const double*)partials, g_feat);
    }
    hipLaunchKernelGGL(smpl_frame_chain_backward_kernel<POSE>, dim3(1), dim3(SF_BLOCK), 0, s, a->J, smpl_parents(a), a->saved, a->g_A_obs,
                       (const double*)g_feat, a->J > 1 ? a->g_correct_Rs : nullptr, poses, cR, g_poses);
    return launch_status(who);
}

}  // namespace

}  // namespace moss

using namespace moss;

extern "C" size_t moss_smpl_frame_workspace_bytes(int P, int V, int J)
{
    if (P <= 0 || V <= 0 || J < 1 || J > SMPL_MAX_J) return 0;
    return std::max(sf_forward_bytes(V, J), sf_backward_bytes(P, J));
}

extern "C" int moss_smpl_frame_forward(const moss_smpl_frame_args* a, void* stream)
{
    const char* who = "moss_smpl_frame_forward";
    if (!a) return invalid_arg(who, "null argument block");
    if (a->P < 0) return invalid_arg(who, "P must be >= 0");
    if (a->V < 1) return invalid_arg(who, "V must be >= 1");
    if (a->J < 1 || a->J > SMPL_MAX_J) return invalid_arg(who, "J must be 1..64");
    if (a->num_betas_big < 0 || a->num_betas < 0 || a->num_betas_big > a->shapedirs_stride || a->num_betas > a->shapedirs_stride)
        return invalid_arg(who, "num_betas and num_betas_big must be 0..shapedirs_stride");
    if (!a->v_template || !a->shapedirs || !a->J_regressor || !a->poses_big || !a->poses || (a->J > 1 && !a->posedirs))
        return invalid_arg(who, "null required input (v_template, shapedirs, posedirs, J_regressor, poses_big, poses)");
    if ((a->num_betas_big > 0 && !a->shapes_big) || (a->num_betas > 0 && !a->shapes)) return invalid_arg(who, "null shapes");
    if (a->P > 0 && (!a->vert_ids || !a->d)) return invalid_arg(who, "null vert_ids or d");
    if (!a->A_big || !a->A_obs || !a->rot_mats) return invalid_arg(who, "null output (A_big, A_obs, rot_mats)");
    if (int rc = smpl_check_parents(who, a->J, a->parents)) return rc;
    if (!a->workspace || a->workspace_bytes < sf_forward_bytes(a->V, a->J))
        return invalid_arg(who, "needs moss_smpl_frame_workspace_bytes(max(P, 1), V, J) bytes of workspace");
    hipStream_t s = (hipStream_t)stream;
    const SfIn in{a->P, a->V, a->J, a->num_betas_big, a->num_betas, a->shapedirs_stride, a->v_template, a->shapedirs, a->posedirs,
                  a->J_regressor, a->poses_big, a->shapes_big, a->poses, a->shapes, a->correct_Rs, a->vert_ids};
    const SmplParents par = smpl_parents(a);
    float* D = reinterpret_cast<float*>(a->workspace);
    double* partials = reinterpret_cast<double*>(a->workspace + align_up((size_t)a->V * 3 * sizeof(float)));
    const int nparts = (a->V + SMPL_VPB - 1) / SMPL_VPB;
    hipLaunchKernelGGL(smpl_frame_offsets_kernel, dim3(nparts), dim3(SF_BLOCK), 0, s, in, D, partials);
    hipLaunchKernelGGL(smpl_frame_chain_gather_kernel, dim3(1 + (a->P + SF_CHAIN_BLOCK - 1) / SF_CHAIN_BLOCK), dim3(SF_CHAIN_BLOCK), 0, s,
                       in, par, nparts, (const double*)partials, (const float*)D, a->A_big, a->A_obs, a->d, a->rot_mats, a->saved);
    return launch_status(who);
}

extern "C" int moss_smpl_frame_backward(const moss_smpl_frame_backward_args* a, void* stream)
{
    return sf_backward_impl<false>("moss_smpl_frame_backward", a, stream);
}

extern "C" int moss_smpl_frame_backward_pose(const moss_smpl_frame_backward_pose_args* a, void* stream)
{
    return sf_backward_impl<true>("moss_smpl_frame_backward_pose", a, stream);
}
