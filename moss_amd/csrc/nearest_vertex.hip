// nearest_vertex.hip -- the nearest template vertex of every query point: exact, k = 1, against a vertex set that never changes.
//
// MOSS asks, on every training step, for the nearest SMPL vertex of every Gaussian (scene/gaussian_model.py:827: knn(t_vertices,
// query_pts), V = 6 890 vertices of the big pose, the same every step) and, when pruning, for the distance to it (:657).  The cell
// grid of knn_query.hip answers that with one thread per query walking shells of mostly empty cells (the template is a surface) and
// is rebuilt on every call.  Here the vertices are indexed ONCE per subject and a query is one launch:
//
//   index   the vertices sorted along a Morton curve of their bounding box and cut into blocks of 64; each vertex stored as
//           (x, y, z, original index as int bits), each block with its axis-aligned box.  A snapshot: later changes of the vertex
//           tensor are not seen.  Built on the device, three launches, no host read; not on the hot path, so the sort is a rank by
//           counting (every vertex counts the keys below its own: V^2 comparisons, 0.1 ms at V = 65 536).
//   query   a GROUP of 16 lanes works on one query at a time, four groups to a wave.  The boxes sit in LDS.  Pass 1: the lanes take
//           the boxes and find the one nearest to the query; its 64 vertices are evaluated, four per lane.  Pass 2: the lanes take the
//           boxes again, a ballot keeps the blocks whose lower bound is not above the best distance so far, and the group evaluates
//           them one by one, re-testing each against the bound as it has tightened meanwhile.  Every lane keeps its own best (d, id);
//           one arg-min over the group ends the query.  The cost barely depends on the order of the queries: a group never
//           evaluates another group's blocks, it only waits while the wave's other three finish theirs.
//
// EXACT: d is the brute-force kernel's expression (nearest_vertex_math.h: dist2; this file is compiled with -ffp-contract=off like
// knn_query.hip), candidates are ordered by (d, vertex index) explicitly, and a block is skipped only when its lower bound -- which
// is never above the computed d of any vertex inside, see the header -- is STRICTLY greater than the best d.  So ids and distances
// equal moss_knn_query(k = 1) bit for bit, ties included.  A query with a non-finite coordinate gets id -1 and distance +inf, as
// there (no d is below +inf).  Every loop runs over the block count; nothing depends on the data to end.
#include "common.h"
#include "wave.h"
#include "nearest_vertex_math.h"

namespace moss {
namespace {

namespace nv = nearest_vertex;

constexpr int NV_KEY_TILE = 1024;

struct IndexView {
    uint64_t* keys; float4* verts; float4* boxes;    // keys: the build's scratch; verts: NB * 64 (the tail of the last block is padding,
    int NB;                                          // never read as a vertex); boxes: {lo.xyz, -}, {hi.xyz, -} per block
    static IndexView at(char* base, int V)
    {
        IndexView v; char* p = base;
        v.NB = nv::blocks_for(V);
        v.keys = carve<uint64_t>(p, (size_t)V);
        v.verts = carve<float4>(p, (size_t)v.NB * nv::BLOCK);
        v.boxes = carve<float4>(p, 2 * (size_t)v.NB);
        return v;
    }
    static size_t bytes(int V) { char* z = nullptr; IndexView v = at(z, V); return (size_t)((char*)v.boxes - z) + align_up(2 * (size_t)v.NB * sizeof(float4)); }
};

// ---- build ---------------------------------------------------------------------------------------------------------------------
// one workgroup: the bounding box (finite or not; NaN coordinates are dropped by fminf / fmaxf), then every vertex's sort key
__global__ void __launch_bounds__(1024)
nv_keys_kernel(int V, const float* __restrict__ pts, uint64_t* __restrict__ keys)
{
    __shared__ float s_mn[16][3], s_mx[16][3];
    __shared__ float s_lo[3], s_hi[3];
    float mn[3] = { __builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf() };
    float mx[3] = { -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf() };
    for (int i = threadIdx.x; i < V; i += blockDim.x)
#pragma unroll
        for (int k = 0; k < 3; k++) { const float v = pts[3 * (size_t)i + k]; mn[k] = fminf(mn[k], v); mx[k] = fmaxf(mx[k], v); }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mn[k] = wave_min(mn[k]); mx[k] = wave_max(mx[k]);
        if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6][k] = mn[k]; s_mx[threadIdx.x >> 6][k] = mx[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        float lo = s_mn[0][k], hi = s_mx[0][k];
        for (int w = 1; w < 16; w++) { lo = fminf(lo, s_mn[w][k]); hi = fmaxf(hi, s_mx[w][k]); }
        s_lo[k] = lo; s_hi[k] = hi;
    }
    __syncthreads();
    const float lo[3] = { s_lo[0], s_lo[1], s_lo[2] }, hi[3] = { s_hi[0], s_hi[1], s_hi[2] };
    for (int i = threadIdx.x; i < V; i += blockDim.x)
        keys[i] = nv::morton_key(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], lo, hi, (uint32_t)i);
}

// vertex i goes to slot rank(i) = the number of keys below its own (keys are unique: the ranks are a permutation of 0 .. V-1);
// the threads past V fill the padding of the last block
__global__ void __launch_bounds__(256)
nv_rank_scatter_kernel(int V, int slots, const float* __restrict__ pts, const uint64_t* __restrict__ keys, float4* __restrict__ verts)
{
    __shared__ uint64_t s_keys[NV_KEY_TILE];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t mine = i < V ? keys[i] : 0ull;
    uint32_t rank = 0;
    for (int base = 0; base < V; base += NV_KEY_TILE) {
        const int cnt = min(NV_KEY_TILE, V - base);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += blockDim.x) s_keys[j] = keys[base + j];
        __syncthreads();
        for (int j = 0; j < cnt; j++) rank += s_keys[j] < mine ? 1u : 0u;
    }
    if (i < V) {
        if (rank < (uint32_t)V)
            verts[rank] = make_float4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], __int_as_float(i));
    } else if (i < slots) {
        verts[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    }
}

// one wave per block: the exact minimum and maximum of its vertices' coordinates
__global__ void __launch_bounds__(256)
nv_boxes_kernel(int V, int NB, const float4* __restrict__ verts, float4* __restrict__ boxes)
{
    const int b = blockIdx.x * (blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (b >= NB) return;                                                       // (whole waves leave: b is wave-uniform)
    const int i = b * nv::BLOCK + (int)(threadIdx.x & 63);
    float lo[3] = { __builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf() };
    float hi[3] = { -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf() };
    if (i < V) { const float4 v = verts[i]; lo[0] = hi[0] = v.x; lo[1] = hi[1] = v.y; lo[2] = hi[2] = v.z; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        // (a NaN coordinate: lo = hi = NaN in its lane, dropped by the reductions' fminf / fmaxf unless the whole block is NaN --
        // put it back to the empty interval then, so that the box never holds a NaN)
        lo[k] = wave_min(lo[k]); hi[k] = wave_max(hi[k]);
        if (!(lo[k] == lo[k])) lo[k] = __builtin_huge_valf();
        if (!(hi[k] == hi[k])) hi[k] = -__builtin_huge_valf();
    }
    if ((threadIdx.x & 63) == 0) {
        boxes[2 * (size_t)b] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[2 * (size_t)b + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------
// A GROUP of 16 lanes -- one DPP row -- works on a query; the four groups of a wave work on four queries side by side.  A query is a
// chain of dependent steps (its point, the nearest box, that block's vertices, the bound, the next block ...), each a memory round
// trip, so a wave that held ONE query spent its time waiting (measured, 45 695 queries in spatial order: 62 us with a wave per query
// and ds_bpermute reductions, 37 us this way); here four chains run per wave and the reductions stay inside the row (DPP: no LDS round trip).
constexpr int GROUP = 16;
constexpr int PER_LANE = nv::BLOCK / GROUP;           // vertices of a block per lane

template <int CTRL>
__device__ __forceinline__ int row_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
// rotations by 8, 4, 2, 1 inside the row of 16 lanes (DPP row_ror): after the four steps every lane holds the row's result
#define MOSS_ROW_REDUCE(v, op, cast_in, cast_out)                                                   \
    v = op(v, cast_out(row_dpp<0x128>(cast_in(v)))); v = op(v, cast_out(row_dpp<0x124>(cast_in(v)))); \
    v = op(v, cast_out(row_dpp<0x122>(cast_in(v)))); v = op(v, cast_out(row_dpp<0x121>(cast_in(v))));
__device__ __forceinline__ float row_min(float v) { MOSS_ROW_REDUCE(v, fminf, __float_as_int, __int_as_float) return v; }
__device__ __forceinline__ int row_min(int v) { MOSS_ROW_REDUCE(v, min, , ) return v; }
#undef MOSS_ROW_REDUCE

// the group evaluates one block: lane l takes vertices l, l + 16, l + 32, l + 48 of it (four independent loads)
__device__ __forceinline__ void eval_block(const float4* __restrict__ verts, int V, int block, int l, float qx, float qy, float qz,
                                           float& bd, int& bi)
{
    const int i0 = block * nv::BLOCK + l;
    float4 v[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) v[k] = verts[i0 + k * GROUP];           // (inside the padded array whatever V is)
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const float d = nv::dist2(v[k].x, v[k].y, v[k].z, qx, qy, qz);
        const int id = __float_as_int(v[k].w);
        if (i0 + k * GROUP < V && nv::closer(d, id, bd, bi)) { bd = d; bi = id; }
    }
}

__global__ void __launch_bounds__(256)
nv_query_kernel(int V, int NB, int P, const float4* __restrict__ verts, const float4* __restrict__ boxes, const float* __restrict__ points,
                long long* __restrict__ ids_out, float* __restrict__ dist_out)
{
    extern __shared__ float4 s_box[];                                          // 2 * NB
    for (int j = threadIdx.x; j < 2 * NB; j += blockDim.x) s_box[j] = boxes[j];
    __syncthreads();
    const int l = (int)(threadIdx.x & (GROUP - 1));                            // lane of the group
    const int row = (int)(threadIdx.x & 63) / GROUP;                           // group of the wave
    const int groups = (int)(gridDim.x * (blockDim.x / GROUP));
    for (int q = (int)(blockIdx.x * (blockDim.x / GROUP) + threadIdx.x / GROUP); q < P; q += groups) {      // (q is group-uniform)
        const float qx = points[3 * (size_t)q], qy = points[3 * (size_t)q + 1], qz = points[3 * (size_t)q + 2];
        float bd = __builtin_huge_valf();
        int bi = -1;
        if (fabsf(qx) < __builtin_huge_valf() && fabsf(qy) < __builtin_huge_valf() && fabsf(qz) < __builtin_huge_valf()) {
            // pass 1: the box nearest to the query (the lowest block among equals)
            float mlb = __builtin_huge_valf();
            int mb = 0x7fffffff;
            for (int j = l; j < NB; j += GROUP) {
                const float4 lo = s_box[2 * j], hi = s_box[2 * j + 1];
                const float lb = nv::box_lower_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qx, qy, qz);
                if (lb < mlb) { mlb = lb; mb = j; }
            }
            const float m = row_min(mlb);                                      // (every mlb is a number: nothing here forms a NaN)
            const int first = min(row_min(mlb == m ? mb : 0x7fffffff), NB - 1); // 0 <= first < NB (NB - 1: no box has a finite bound)
            eval_block(verts, V, first, l, qx, qy, qz, bd, bi);
            float best = row_min(bd);                                          // group-uniform: what decides the skips
            // pass 2: every other block whose lower bound is not above the best distance
            for (int base = 0; base < NB; base += GROUP) {
                const int j = base + l;
                float lb = __builtin_huge_valf();
                if (j < NB) {
                    const float4 lo = s_box[2 * j], hi = s_box[2 * j + 1];
                    lb = nv::box_lower_bound(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qx, qy, qz);
                }
                uint32_t todo = (uint32_t)(__ballot(j < NB && j != first && !nv::can_skip(lb, best)) >> (row * GROUP)) & 0xffffu;
                while (todo) {                                                 // (group-uniform; the groups of a wave differ)
                    const int b = __ffs(todo) - 1;
                    todo &= todo - 1;
                    if (nv::can_skip(__shfl(lb, row * GROUP + b), best)) continue;      // the bound has tightened since the ballot
                    eval_block(verts, V, base + b, l, qx, qy, qz, bd, bi);
                    best = row_min(bd);
                }
            }
            // arg-min over the group by (d, id): the least d, then the least id among the lanes that hold it
            bi = row_min(bd == best ? bi : 0x7fffffff);                        // (best == row_min(bd); all +inf: every bi is -1)
            bd = best;
        }
        if (l == 0) {
            ids_out[q] = (long long)bi;
            if (dist_out) dist_out[q] = sqrtf(bd);
        }
    }
}

}  // namespace
}  // namespace moss

extern "C" size_t moss_nearest_vertex_index_bytes(int V)
{
    return (V < 1 || V > moss::nearest_vertex::MAX_V) ? 0 : moss::IndexView::bytes(V);
}

extern "C" int moss_nearest_vertex_build(int V, const float* vertices, char* index, size_t index_bytes, void* stream)
{
    using namespace moss;
    const char* who = "moss_nearest_vertex_build";
    if (V < 1 || V > nv::MAX_V) return invalid_arg(who, "V outside 1 .. 65536");
    if (!vertices) return invalid_arg(who, "null vertices");
    if (!index || index_bytes < IndexView::bytes(V)) return invalid_arg(who, "index missing or shorter than moss_nearest_vertex_index_bytes(V)");
    hipStream_t s = (hipStream_t)stream;
    IndexView v = IndexView::at(index, V);
    const int slots = v.NB * nv::BLOCK;
    hipLaunchKernelGGL(nv_keys_kernel, dim3(1), dim3(1024), 0, s, V, vertices, v.keys);
    hipLaunchKernelGGL(nv_rank_scatter_kernel, dim3((slots + 255) / 256), dim3(256), 0, s, V, slots, vertices, v.keys, v.verts);
    hipLaunchKernelGGL(nv_boxes_kernel, dim3((v.NB + 3) / 4), dim3(256), 0, s, V, v.NB, v.verts, v.boxes);
    return launch_status(who);
}

extern "C" int moss_nearest_vertex_query(int V, int P, const char* index, size_t index_bytes, const float* points, long long* ids_out,
                                         float* dist_out, void* stream)
{
    using namespace moss;
    const char* who = "moss_nearest_vertex_query";
    if (V < 1 || V > nv::MAX_V) return invalid_arg(who, "V outside 1 .. 65536");
    if (P < 0) return invalid_arg(who, "P < 0");
    if (!index || index_bytes < IndexView::bytes(V)) return invalid_arg(who, "index missing or shorter than moss_nearest_vertex_index_bytes(V)");
    if (P == 0) return 0;
    if (!points || !ids_out) return invalid_arg(who, "null points or ids_out");
    IndexView v = IndexView::at(const_cast<char*>(index), V);
    // sixteen lanes per query, sixteen queries per workgroup; enough workgroups to fill the device, each group then strides over the queries
    const int grid = std::min((P + 15) / 16, 8 * device_cus());
    const size_t lds = 2 * (size_t)v.NB * sizeof(float4);                       // <= 32 KiB at V = 65 536
    hipLaunchKernelGGL(nv_query_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, V, v.NB, P, v.verts, v.boxes, points, ids_out,
                       dist_out);
    return launch_status(who);
}
