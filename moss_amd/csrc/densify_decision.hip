// densify_decision.hip -- MOSS's KL densify-and-prune DECISION (GaussianModel.densify_and_prune, scene/gaussian_model.py:621-666, and
// kl_densify_and_clone :495-526, kl_densify_and_split :528-571, kl_merge :573-619) as three entry points:
//
//   moss_densify_joint_table   joint_F / denom[0] -> SVD -> sign rule -> U V^T and S per joint, as the (24,12) table both blends read
//   moss_densify_select        one phase's mask, its ASCENDING index list and its count (one host read per phase: the count)
//   moss_densify_emit          one phase's new rows, written into caller-allocated tensors
//
// The reference does this with ~120 small torch launches per event, a boolean-index host synchronisation at every x[mask], a Python
// loop over P inside kl_div and a (P,3,3) blend of the joint rotations of which only the selected rows are ever read.
//
// The KL of a selection is computed by neighbour_kl_kernel itself (densify.hip, through launch_neighbour_kl) on scales activated here:
// moss_neighbour_kl's bits by construction.
// The row kernel runs one wave per workgroup: every lane owns a new row for the small tensors, then the 64 lanes walk the feature rows.
// Ordered compaction without an order-dependent atomic: launch 1 decides a flag per Gaussian and leaves one total per workgroup (ballot
// + popcount per wave, four wave counts added through LDS); launch 2 gives each workgroup the sum of the totals before it (integers: any
// order gives the same sum), each wave its offset in the workgroup and each lane its rank in the wave (ballot, popcount of the lanes
// below).  Same bits every run.  There is no float atomic in this file.
#include "common.h"
#include "kl_math.h"
#include "pose_math.h"

namespace moss {
namespace {

constexpr int DD_BLOCK = 256;
constexpr int DD_WAVES = DD_BLOCK / 64;
constexpr int DD_J = MOSS_DENSIFY_JOINTS;
constexpr int DD_ROWS = 64;                  // rows of new Gaussians per workgroup of the emit kernel: ONE wave, every lane a row

__global__ void __launch_bounds__(64)
joint_table_kernel(const float* __restrict__ F_sum, const float* __restrict__ denom, float* __restrict__ table)
{
    const int j = threadIdx.x;
    if (j >= DD_J) return;
    float* row = table + 12 * j;
    if (j == 0) {                                                            // torch.ones(1,3,3), torch.ones(1,3) (:637,640)
#pragma unroll
        for (int c = 0; c < 12; c++) row[c] = 1.0f;
        return;
    }
    const float d0 = denom[0];
    float F[9];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 9; c++) {
        F[c] = F_sum[9 * (j - 1) + c] / d0;                                  // (:624)
        finite = finite && isfinite(F[c]);
    }
    if (!finite) {
#pragma unroll
        for (int c = 0; c < 12; c++) row[c] = __builtin_nanf("");
        return;
    }
    pose::Svd3 s;
    pose::svd3(F, s);
    // U[:,2] *= det U, V[:,2] *= det V (:632-633): U V^T becomes U diag(1, 1, det U det V) V^T
    const float d[3] = {1.0f, 1.0f, s.det};
    pose::u_diag_vt(s.U, s.V, d, row);
    row[9] = s.s[0]; row[10] = s.s[1]; row[11] = s.s[2];
}

struct SelectParams {
    int mode, P, n_grads, use_screen_size;
    const float *accum, *denom, *xyz, *rotation, *scaling, *opacity, *max_radii, *vertex_dist;
    const long long* ids;
    const uint8_t* surface;
    float max_grad, scale_limit, kl_threshold, min_opacity, max_screen_size, world_scale_limit, vertex_dist_limit;
    uint8_t* mask;
    int* index;
    int* count;
    const float* act;                        // exp(scaling) (P,3): CLONE / SPLIT / MERGE
    const float* kl;
    int* totals;
};

// exp(_scaling) for the KL kernel, which takes activated scales
__global__ void __launch_bounds__(DD_BLOCK)
activate_scales_kernel(long long n, const float* __restrict__ raw, float* __restrict__ act)
{
    const long long i = (long long)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (i < n) act[i] = expf(raw[i]);
}

__device__ __forceinline__ bool decide(const SelectParams& a, int i)
{
    if (a.mode == MOSS_DENSIFY_PRUNE) {
        const float smax = fmaxf(fmaxf(expf(a.scaling[3 * (size_t)i]), expf(a.scaling[3 * (size_t)i + 1])), expf(a.scaling[3 * (size_t)i + 2]));
        bool sel = 1.0f / (1.0f + expf(-a.opacity[i])) < a.min_opacity;                                  // (:650)
        if (a.use_screen_size) sel = sel || a.max_radii[i] > a.max_screen_size || smax > a.world_scale_limit;   // (:652-654)
        return sel || a.vertex_dist[i] > a.vertex_dist_limit;                                             // (:657-662)
    }
    float g = 0.0f;                                                          // the zero padding beyond n_grads (:540-541)
    if (i < a.n_grads) {
        g = a.accum[i] / a.denom[i];                                         // (:622)
        if (g != g) g = 0.0f;                                                // grads[grads.isnan()] = 0 (:642)
    }
    const float smax = fmaxf(fmaxf(a.act[3 * (size_t)i], a.act[3 * (size_t)i + 1]), a.act[3 * (size_t)i + 2]);   // (activated for the KL kernel already)
    if (a.mode == MOSS_DENSIFY_CLONE) g = fabsf(g);                          // torch.norm(grads, dim=-1) of one column (:499)
    bool sel = g >= a.max_grad && (a.mode == MOSS_DENSIFY_SPLIT ? smax > a.scale_limit : smax <= a.scale_limit);
    if (a.mode == MOSS_DENSIFY_CLONE && a.surface) sel = sel && a.surface[i] != 0;
    const float kl = a.kl[i];                                                // written by neighbour_kl_kernel itself, launched before this kernel
    return sel && (a.mode == MOSS_DENSIFY_MERGE ? kl < a.kl_threshold : kl > a.kl_threshold);
}

__global__ void __launch_bounds__(DD_BLOCK)
select_flags_kernel(SelectParams a)
{
    __shared__ int wave_count[DD_WAVES];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * DD_BLOCK + tid;
    bool flag = false;
    if (i < a.P) {
        flag = decide(a, (int)i);
        a.mask[i] = flag ? 1 : 0;
    }
    const unsigned long long ballot = __ballot(flag);
    if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(ballot);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < DD_WAVES; w++) total += wave_count[w];
        a.totals[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(DD_BLOCK)
select_scatter_kernel(SelectParams a)
{
    __shared__ int red[DD_BLOCK];
    __shared__ int wave_count[DD_WAVES];
    const int tid = threadIdx.x;
    int before = 0;                                                          // the selected Gaussians of the workgroups before this one
    for (int b = tid; b < (int)blockIdx.x; b += DD_BLOCK) before += a.totals[b];
    red[tid] = before;
    __syncthreads();
    for (int s = DD_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const int base = red[0];
    const long long i = (long long)blockIdx.x * DD_BLOCK + tid;
    const bool flag = i < a.P && a.mask[i] != 0;
    const unsigned long long ballot = __ballot(flag);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int wave_base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DD_WAVES; w++) {
        if (w < wave) wave_base += wave_count[w];
        total += wave_count[w];
    }
    if (flag && a.index) a.index[base + wave_base + __popcll(ballot & ((1ull << lane) - 1ull))] = (int)i;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.count = base + total;
}

struct EmitParams {
    int mode, P, n_sel, n_new, rest_floats, dc_stride, rest_stride;
    const int* index;
    const long long* ids;
    const float *xyz, *features_dc, *features_rest, *opacity, *scaling, *rotation, *lbs_weights, *denom, *table, *noise;
    float *new_xyz, *new_features_dc, *new_features_rest, *new_opacity, *new_scaling, *new_rotation;
    uint8_t* prune_mask;
};

// pytorch3d.transforms.matrix_to_quaternion (rotation_conversions.py): q_abs = sqrt(max(0, 1 +- m00 +- m11 +- m22)), the candidate
// built around the largest q_abs, divided by 2 max(q_abs, 0.1); real part first.
__device__ __forceinline__ void matrix_to_quaternion(const float m[9], float q[4])
{
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float t[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    float qa[4];
    int best = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        qa[k] = t[k] > 0.0f ? sqrtf(t[k]) : 0.0f;
        if (qa[k] > qa[best]) best = k;
    }
    float c[4];
    if (best == 0)      { c[0] = qa[0] * qa[0]; c[1] = m21 - m12;       c[2] = m02 - m20;       c[3] = m10 - m01; }
    else if (best == 1) { c[0] = m21 - m12;     c[1] = qa[1] * qa[1];   c[2] = m10 + m01;       c[3] = m02 + m20; }
    else if (best == 2) { c[0] = m02 - m20;     c[1] = m10 + m01;       c[2] = qa[2] * qa[2];   c[3] = m12 + m21; }
    else                { c[0] = m10 - m01;     c[1] = m20 + m02;       c[2] = m21 + m12;       c[3] = qa[3] * qa[3]; }
    const float div = 2.0f * fmaxf(qa[best], 0.1f);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = c[k] / div;
}

__global__ void __launch_bounds__(DD_ROWS)
emit_kernel(EmitParams a)
{
    __shared__ float table[DD_J * 12];
    __shared__ int src_a[DD_ROWS], src_b[DD_ROWS];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * DD_ROWS;
    const int rows = min(DD_ROWS, a.n_new - row0);
    if (a.mode == MOSS_DENSIFY_CLONE) {
        for (int e = tid; e < DD_J * 12; e += DD_ROWS) table[e] = a.table[e];
        __syncthreads();
    }
    if (tid < rows) {                                                        // ---- one lane per new row: everything but the features
        const int r = row0 + tid;
        long long ia = a.index[a.mode == MOSS_DENSIFY_SPLIT ? r % a.n_sel : r], ib = -1;
        if (ia < 0 || ia >= a.P) ia = -1;
        if (a.mode == MOSS_DENSIFY_MERGE && ia >= 0) {
            const long long sel = ia;
            ia = a.ids[2 * sel]; ib = a.ids[2 * sel + 1];                   // selected_point_ids (:606)
            if (ia < 0 || ia >= a.P || ib < 0 || ib >= a.P) ia = ib = -1;
        }
        src_a[tid] = (int)ia; src_b[tid] = (int)ib;
        float nx[3] = {0.f, 0.f, 0.f}, ns[3] = {0.f, 0.f, 0.f}, nq[4] = {0.f, 0.f, 0.f, 0.f}, no = 0.0f;
        if (ia >= 0) {
            float s[3], x[3], q[4];
#pragma unroll
            for (int k = 0; k < 3; k++) { s[k] = expf(a.scaling[3 * ia + k]); x[k] = a.xyz[3 * ia + k]; }
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = a.rotation[4 * ia + k];
            no = a.opacity[ia];
            if (a.mode == MOSS_DENSIFY_MERGE) {
#pragma unroll
                for (int k = 0; k < 3; k++) { nx[k] = (x[k] + a.xyz[3 * ib + k]) / 2.0f; ns[k] = logf(s[k] / 0.8f); }   // (:607-608)
#pragma unroll
                for (int k = 0; k < 4; k++) nq[k] = q[k];                                                               // (:609)
                no = (no + a.opacity[ib]) / 2.0f;                                                                        // (:612)
                a.prune_mask[ib] = 1;                                        // (:616; several lanes may store the same 1)
            } else {
                float R[3][3], M[3][3], std[3];
                rotation_of(q, R);
                const float* nz = a.noise + 3 * (size_t)r;
                if (a.mode == MOSS_DENSIFY_SPLIT) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        std[k] = s[k]; ns[k] = logf(s[k] / 1.6f);           // get_scaling / (0.8 N), N = 2 (:560)
#pragma unroll
                        for (int c = 0; c < 3; c++) M[k][c] = R[k][c];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) nq[k] = q[k];
                } else {
                    const float d0 = a.denom[0];
                    float blend[12];
#pragma unroll
                    for (int c = 0; c < 12; c++) blend[c] = 0.0f;
                    for (int j = 0; j < DD_J; j++) {                         // lbs_weights[0] @ rot_joint, @ scl_joint (:638,641)
                        const float w = a.lbs_weights[(size_t)DD_J * ia + j] / d0;     // (:625)
#pragma unroll
                        for (int c = 0; c < 12; c++) blend[c] += w * table[12 * j + c];
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        std[k] = blend[9 + k] * s[k];                        // (:511)
                        ns[k] = logf(s[k] * blend[9 + k]);                   // (:519)
#pragma unroll
                        for (int c = 0; c < 3; c++)                          // rot_joint @ build_rotation(q) (:517)
                            M[k][c] = blend[3 * k] * R[0][c] + blend[3 * k + 1] * R[1][c] + blend[3 * k + 2] * R[2][c];
                    }
                    float qj[4];
                    matrix_to_quaternion(blend, qj);
#pragma unroll
                    for (int k = 0; k < 4; k++) nq[k] = qj[k] * q[k];        // ELEMENTWISE, as :520
                }
#pragma unroll
                for (int k = 0; k < 3; k++)                                  // bmm(rots, samples) + xyz (:518,558)
                    nx[k] = (M[k][0] * (std[0] * nz[0]) + M[k][1] * (std[1] * nz[1]) + M[k][2] * (std[2] * nz[2])) + x[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) { a.new_xyz[3 * (size_t)r + k] = nx[k]; a.new_scaling[3 * (size_t)r + k] = ns[k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) a.new_rotation[4 * (size_t)r + k] = nq[k];
        a.new_opacity[r] = no;
    }
    __syncthreads();
    // ---- the feature rows: lanes along the 3 + rest_floats floats of a row
    const int F = 3 + a.rest_floats;
    for (int e = tid; e < rows * F; e += DD_ROWS) {
        const int lr = e / F, c = e - lr * F;
        const int ia = src_a[lr], ib = src_b[lr];
        const float* base = c < 3 ? a.features_dc + c : a.features_rest + (c - 3);
        const size_t stride = c < 3 ? a.dc_stride : a.rest_stride;
        float v = 0.0f;
        if (ia >= 0) {
            v = base[(size_t)ia * stride];
            if (a.mode == MOSS_DENSIFY_MERGE) v = (v + base[(size_t)ib * stride]) / 2.0f;               // (:610-611)
        }
        const size_t r = (size_t)(row0 + lr);
        if (c < 3) a.new_features_dc[3 * r + c] = v;
        else a.new_features_rest[(size_t)a.rest_floats * r + (c - 3)] = v;
    }
}

inline int select_blocks(int P) { return P <= 0 ? 0 : (P - 1) / DD_BLOCK + 1; }

}  // namespace
}  // namespace moss

using namespace moss;

extern "C" int moss_densify_joint_table(const float* joint_F_sum, const float* denom, float* table, void* stream)
{
    const char* who = "moss_densify_joint_table";
    if (!joint_F_sum || !denom || !table) return invalid_arg(who, "null joint_F_sum, denom or table");
    hipLaunchKernelGGL(joint_table_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, joint_F_sum, denom, table);
    return launch_status(who);
}

// workspace: one total per workgroup (all PRUNE needs), then the activated scales (3 P floats) and the KL (P floats; unused when the
// caller gives kl_out)
inline size_t totals_bytes(int P) { return (size_t)std::max(select_blocks(P), 1) * sizeof(int); }

extern "C" size_t moss_densify_select_workspace_bytes(int P)
{
    return totals_bytes(P) + (size_t)std::max(P, 0) * 4 * sizeof(float);
}

extern "C" int moss_densify_select(const moss_densify_select_args* x, void* stream)
{
    const char* who = "moss_densify_select";
    if (!x) return invalid_arg(who, "null argument block");
    if (x->mode < MOSS_DENSIFY_CLONE || x->mode > MOSS_DENSIFY_PRUNE) return invalid_arg(who, "unknown mode");
    if (x->P < 0 || x->n_grads < 0 || x->n_grads > x->P) return invalid_arg(who, "P < 0 or n_grads outside [0, P]");
    if (!x->count) return invalid_arg(who, "null count");
    hipStream_t s = (hipStream_t)stream;
    if (x->P > 0) {
        if (!x->mask || !x->scaling) return invalid_arg(who, "null mask or scaling");
        if (x->mode == MOSS_DENSIFY_PRUNE) {
            if (!x->opacity || !x->vertex_dist) return invalid_arg(who, "PRUNE needs opacity and vertex_dist");
            if (x->use_screen_size && !x->max_radii2D) return invalid_arg(who, "use_screen_size needs max_radii2D");
        } else {
            if (!x->xyz || !x->rotation || !x->ids) return invalid_arg(who, "null xyz, rotation or ids");
            if (x->n_grads > 0 && (!x->xyz_gradient_accum || !x->denom)) return invalid_arg(who, "null xyz_gradient_accum or denom");
        }
        if (!x->workspace || x->workspace_bytes < (x->mode == MOSS_DENSIFY_PRUNE ? totals_bytes(x->P) : moss_densify_select_workspace_bytes(x->P)))
            return invalid_arg(who, "workspace missing or too small");
        SelectParams a = {};
        a.mode = x->mode; a.P = x->P; a.n_grads = x->n_grads; a.use_screen_size = x->use_screen_size;
        a.accum = x->xyz_gradient_accum; a.denom = x->denom; a.xyz = x->xyz; a.rotation = x->rotation; a.scaling = x->scaling;
        a.opacity = x->opacity; a.max_radii = x->max_radii2D; a.vertex_dist = x->vertex_dist; a.ids = x->ids;
        a.surface = x->mode == MOSS_DENSIFY_CLONE ? x->surface_mask : nullptr;
        a.max_grad = x->max_grad; a.scale_limit = x->scale_limit; a.kl_threshold = x->kl_threshold; a.min_opacity = x->min_opacity;
        a.max_screen_size = x->max_screen_size; a.world_scale_limit = x->world_scale_limit; a.vertex_dist_limit = x->vertex_dist_limit;
        a.mask = x->mask; a.index = x->index; a.count = x->count;
        a.totals = reinterpret_cast<int*>(x->workspace);
        float* act = reinterpret_cast<float*>(x->workspace + totals_bytes(x->P));
        float* kl = x->kl_out ? x->kl_out : act + 3 * (size_t)x->P;
        a.act = act; a.kl = kl;
        const int blocks = select_blocks(x->P);
        if (x->mode != MOSS_DENSIFY_PRUNE) {
            // the KL comes from moss_neighbour_kl's OWN kernel on exp(scaling): the same machine code, hence the same bits; an index
            // of ids outside [0,P) gives NaN there, which no threshold test selects
            hipLaunchKernelGGL(activate_scales_kernel, dim3((unsigned)((3LL * x->P - 1) / DD_BLOCK + 1)), dim3(DD_BLOCK), 0, s, 3LL * x->P, x->scaling, act);
            const int rc = launch_neighbour_kl(x->P, x->P, x->xyz, x->rotation, act, x->ids, kl, s);
            if (rc != 0) return rc;
        }
        hipLaunchKernelGGL(select_flags_kernel, dim3(blocks), dim3(DD_BLOCK), 0, s, a);
        hipLaunchKernelGGL(select_scatter_kernel, dim3(blocks), dim3(DD_BLOCK), 0, s, a);
    } else if (hipMemsetAsync(x->count, 0, sizeof(int), s) != hipSuccess) {
        return launch_status(who);
    }
    if (x->count_host && hipMemcpyAsync(x->count_host, x->count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return launch_status(who);
    return launch_status(who);
}

extern "C" int moss_densify_emit(const moss_densify_emit_args* x, void* stream)
{
    const char* who = "moss_densify_emit";
    if (!x) return invalid_arg(who, "null argument block");
    if (x->mode < MOSS_DENSIFY_CLONE || x->mode > MOSS_DENSIFY_MERGE) return invalid_arg(who, "unknown mode");
    if (x->P < 0 || x->n_sel < 0 || x->n_sel > x->P) return invalid_arg(who, "P < 0 or n_sel outside [0, P]");
    if ((long long)x->n_new != (long long)x->n_sel * (x->mode == MOSS_DENSIFY_SPLIT ? 2 : 1)) return invalid_arg(who, "n_new is not n_sel (2 n_sel for SPLIT)");
    if (x->rest_floats < 0 || x->dc_stride < 3 || x->rest_stride < x->rest_floats) return invalid_arg(who, "rest_floats < 0 or a feature stride shorter than its row");
    if (x->n_new == 0) return 0;
    if (!x->index || !x->xyz || !x->features_dc || !x->opacity || !x->scaling || !x->rotation || (x->rest_floats > 0 && !x->features_rest))
        return invalid_arg(who, "null index or source tensor");
    if (!x->new_xyz || !x->new_features_dc || !x->new_opacity || !x->new_scaling || !x->new_rotation || (x->rest_floats > 0 && !x->new_features_rest))
        return invalid_arg(who, "null destination tensor");
    if (x->mode == MOSS_DENSIFY_MERGE && (!x->ids || !x->prune_mask)) return invalid_arg(who, "MERGE needs ids and prune_mask");
    if (x->mode != MOSS_DENSIFY_MERGE && !x->noise) return invalid_arg(who, "CLONE and SPLIT need noise");
    if (x->mode == MOSS_DENSIFY_CLONE && (!x->lbs_weights || !x->denom || !x->table)) return invalid_arg(who, "CLONE needs lbs_weights, denom and table");
    EmitParams a;
    a.mode = x->mode; a.P = x->P; a.n_sel = x->n_sel; a.n_new = x->n_new; a.rest_floats = x->rest_floats; a.dc_stride = x->dc_stride; a.rest_stride = x->rest_stride;
    a.index = x->index; a.ids = x->ids; a.xyz = x->xyz; a.features_dc = x->features_dc; a.features_rest = x->features_rest;
    a.opacity = x->opacity; a.scaling = x->scaling; a.rotation = x->rotation; a.lbs_weights = x->lbs_weights; a.denom = x->denom;
    a.table = x->table; a.noise = x->noise; a.new_xyz = x->new_xyz; a.new_features_dc = x->new_features_dc;
    a.new_features_rest = x->new_features_rest; a.new_opacity = x->new_opacity; a.new_scaling = x->new_scaling;
    a.new_rotation = x->new_rotation; a.prune_mask = x->prune_mask;
    hipLaunchKernelGGL(emit_kernel, dim3((x->n_new - 1) / DD_ROWS + 1), dim3(DD_ROWS), 0, (hipStream_t)stream, a);
    return launch_status(who);
}
