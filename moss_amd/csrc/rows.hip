// rows.hip -- carrying a densification decision OUT: the row changes of one event as one gather pass (include/moss_raster.h):
//
//   moss_rows_keep_map   the rows that survive a prune mask, ascending, followed by the appended rows' indices: the ROW MAP
//   moss_rows_relayout   every parameter tensor and both AdamW moments of each, gathered through that map from the old flat buffers
//                        into the new ones -- kept rows copied, appended rows with zero moments, alignment gaps zeroed -- in ONE launch
//
// MOSS does this one tensor at a time with boolean indexing and torch.cat (_prune_optimizer, scene/gaussian_model.py:377-394,
// prune_points :396-411, cat_tensors_to_optimizer :413-434, densification_postfix :436-454).
//
// The gather runs with the lanes along the DESTINATION's flat elements: a wave stores 256 contiguous bytes per instruction, and
// because the maps are ascending or near-ascending neighbouring lanes read neighbouring addresses too (a lane per row would put the
// 64 lanes of a wave in 64 different rows).  One grid covers all tensors: a workgroup finds its tensor in a prefix table that
// travels in the kernel arguments.  The compaction is densify_decision.hip's: per-workgroup totals, summed by every workgroup for
// itself, ranks from ballots -- integers only, no atomic, the same map every run.
#include "common.h"

#include <algorithm>
#include <string>
#include <vector>

namespace moss {
namespace {

constexpr int RW_BLOCK = 256;
constexpr int RW_WAVES = RW_BLOCK / 64;
constexpr int RW_PER_THREAD = 4;                       // elements per thread of the gather, RW_BLOCK apart
constexpr int RW_TILE = RW_BLOCK * RW_PER_THREAD;      // flat elements per workgroup

inline int map_blocks(int rows) { return rows <= 0 ? 0 : (rows - 1) / RW_BLOCK + 1; }

__global__ void __launch_bounds__(RW_BLOCK)
keep_totals_kernel(int rows_old, const uint8_t* __restrict__ remove_mask, int* __restrict__ totals)
{
    __shared__ int wave_count[RW_WAVES];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * RW_BLOCK + tid;
    const bool keep = i < rows_old && (!remove_mask || remove_mask[i] == 0);
    const unsigned long long ballot = __ballot(keep);
    if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(ballot);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < RW_WAVES; w++) total += wave_count[w];
        totals[blockIdx.x] = total;
    }
}

// workgroups [0, blocks_old): the kept rows of their 256; workgroups behind them: 256 appended rows each, placed after ALL kept rows.
// The first of those also writes the count (there is always one, also for rows_app == 0).
__global__ void __launch_bounds__(RW_BLOCK)
keep_scatter_kernel(int rows_old, int rows_app, int blocks_old, const uint8_t* __restrict__ remove_mask, const int* __restrict__ totals,
                    int* __restrict__ map_out, int* __restrict__ count_out)
{
    __shared__ int red[RW_BLOCK];
    __shared__ int wave_count[RW_WAVES];
    const int tid = threadIdx.x;
    const int n_before = min((int)blockIdx.x, blocks_old);
    int before = 0;                                                          // the kept rows of the workgroups before this one
    for (int b = tid; b < n_before; b += RW_BLOCK) before += totals[b];
    red[tid] = before;
    __syncthreads();
    for (int s = RW_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const int base = red[0];
    if ((int)blockIdx.x >= blocks_old) {
        const long long j = (long long)((int)blockIdx.x - blocks_old) * RW_BLOCK + tid;
        if (j < rows_app) map_out[base + j] = rows_old + (int)j;
        if ((int)blockIdx.x == blocks_old && tid == 0) *count_out = base + rows_app;
        return;
    }
    const long long i = (long long)blockIdx.x * RW_BLOCK + tid;
    const bool keep = i < rows_old && (!remove_mask || remove_mask[i] == 0);
    const unsigned long long ballot = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int wave_base = 0;
#pragma unroll
    for (int w = 0; w < RW_WAVES; w++)
        if (w < wave) wave_base += wave_count[w];
    if (keep) map_out[base + wave_base + __popcll(ballot & ((1ull << lane) - 1ull))] = (int)i;
}

struct RelayoutTensor {
    const float *src, *src_m, *src_v, *app;
    float *dst, *dst_m, *dst_v;
    int width, use_map;
    unsigned n_body, n_total;                          // rows * width; the same plus pad_after
};

struct RelayoutParams {
    int rows_old, rows_app, num_tensors;
    const int* map;
    int block_start[MOSS_ROWS_MAX_TENSORS + 1];        // first workgroup of each tensor; [num_tensors] = the grid
    RelayoutTensor t[MOSS_ROWS_MAX_TENSORS];
};

// where element e of the destination comes from: 0 a row of src (with its moments), 1 a row of app (zero moments), 2 zeros (the
// alignment gap, a map entry out of range); nothing (3) beyond the tensor
__device__ __forceinline__ int locate(const RelayoutParams& a, const RelayoutTensor& t, unsigned e, size_t& at)
{
    if (e >= t.n_total) return 3;
    if (e >= t.n_body) return 2;
    if (!t.use_map) { at = e; return 0; }
    const unsigned r = e / (unsigned)t.width, c = e - r * (unsigned)t.width;
    const int s = a.map[r];
    if (s < 0 || s >= a.rows_old + a.rows_app) return 2;
    if (s < a.rows_old) { at = (size_t)s * t.width + c; return 0; }
    at = (size_t)(s - a.rows_old) * t.width + c;
    return 1;
}

template <bool MOMENTS>
__device__ __forceinline__ void relayout_tile(const RelayoutParams& a, const RelayoutTensor& t, unsigned e0)
{
    float x[RW_PER_THREAD], m[RW_PER_THREAD], v[RW_PER_THREAD];
    int kind[RW_PER_THREAD];
    // every load of the thread's elements is issued before the first store: three arrays x RW_PER_THREAD loads in flight
#pragma unroll
    for (int k = 0; k < RW_PER_THREAD; k++) {
        size_t at = 0;
        kind[k] = locate(a, t, e0 + k * RW_BLOCK, at);
        x[k] = m[k] = v[k] = 0.0f;
        if (kind[k] == 0) {
            x[k] = t.src[at];
            if (MOMENTS) { m[k] = t.src_m[at]; v[k] = t.src_v[at]; }
        } else if (kind[k] == 1) {
            x[k] = t.app[at];
        }
    }
#pragma unroll
    for (int k = 0; k < RW_PER_THREAD; k++) {
        if (kind[k] == 3) continue;
        const unsigned e = e0 + k * RW_BLOCK;
        t.dst[e] = x[k];
        if (MOMENTS) { t.dst_m[e] = m[k]; t.dst_v[e] = v[k]; }
    }
}

__global__ void __launch_bounds__(RW_BLOCK)
rows_relayout_kernel(RelayoutParams a)
{
    int ti = 0;                                                              // (uniform: the whole workgroup is in one tensor)
#pragma unroll
    for (int k = 1; k < MOSS_ROWS_MAX_TENSORS; k++)
        if (k < a.num_tensors && (int)blockIdx.x >= a.block_start[k]) ti = k;
    const RelayoutTensor& t = a.t[ti];
    const unsigned e0 = (unsigned)((int)blockIdx.x - a.block_start[ti]) * RW_TILE + threadIdx.x;
    if (t.dst_m) relayout_tile<true>(a, t, e0);
    else relayout_tile<false>(a, t, e0);
}

struct Range { const char* lo; const char* hi; std::string name; };

inline bool overlap(const Range& a, const Range& b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

}  // namespace
}  // namespace moss

using namespace moss;

extern "C" size_t moss_rows_map_workspace_bytes(int rows_old)
{
    return (size_t)std::max(map_blocks(rows_old), 1) * sizeof(int);
}

extern "C" int moss_rows_keep_map(int rows_old, const uint8_t* remove_mask, int rows_app, int* map_out, int* count_out, char* workspace,
                                  size_t workspace_bytes, void* stream)
{
    const char* who = "moss_rows_keep_map";
    if (rows_old < 0 || rows_app < 0 || (long long)rows_old + rows_app > 0x7fffffffLL) return invalid_arg(who, "rows_old < 0, rows_app < 0 or their sum beyond int32");
    if (!count_out) return invalid_arg(who, "null count_out");
    if (!map_out && rows_old + rows_app > 0) return invalid_arg(who, "null map_out");
    if (!workspace || workspace_bytes < moss_rows_map_workspace_bytes(rows_old)) return invalid_arg(who, "workspace missing or too small");
    hipStream_t s = (hipStream_t)stream;
    int* totals = reinterpret_cast<int*>(workspace);
    const int blocks_old = map_blocks(rows_old), blocks_app = std::max(map_blocks(rows_app), 1);
    if (blocks_old > 0) hipLaunchKernelGGL(keep_totals_kernel, dim3(blocks_old), dim3(RW_BLOCK), 0, s, rows_old, remove_mask, totals);
    hipLaunchKernelGGL(keep_scatter_kernel, dim3(blocks_old + blocks_app), dim3(RW_BLOCK), 0, s, rows_old, rows_app, blocks_old, remove_mask,
                       (const int*)totals, map_out, count_out);
    return launch_status(who);
}

extern "C" int moss_rows_relayout(const moss_rows_relayout_args* x, void* stream)
{
    const char* who = "moss_rows_relayout";
    if (!x) return invalid_arg(who, "null argument block");
    if (x->rows_old < 0 || x->rows_app < 0 || x->rows_new < 0) return invalid_arg(who, "rows_old, rows_app or rows_new < 0");
    if ((long long)x->rows_old + x->rows_app > 0x7fffffffLL) return set_last_error(MOSS_ERR_UNSUPPORTED, (std::string(who) + ": rows_old + rows_app beyond int32").c_str());
    if (x->num_tensors < 0) return invalid_arg(who, "num_tensors < 0");
    if (x->num_tensors > MOSS_ROWS_MAX_TENSORS)
        return set_last_error(MOSS_ERR_UNSUPPORTED, (std::string(who) + ": num_tensors above MOSS_ROWS_MAX_TENSORS").c_str());
    if (x->rows_new > 0 && !x->map) return invalid_arg(who, "null map");

    RelayoutParams a = {};
    a.rows_old = x->rows_old; a.rows_app = x->rows_app; a.num_tensors = x->num_tensors; a.map = x->map;
    std::vector<Range> sources, dests;
    auto bytes = [](const void* p, size_t floats, std::string name) {
        return Range{static_cast<const char*>(p), static_cast<const char*>(p) + floats * sizeof(float), std::move(name)};
    };
    if (x->map) sources.push_back(bytes(x->map, (size_t)x->rows_new, "map"));
    long long grid = 0;
    for (int i = 0; i < x->num_tensors; i++) {
        const moss_rows_tensor& d = x->tensors[i];
        const std::string tag = "tensors[" + std::to_string(i) + "].";
        auto refuse = [&](const char* field, const char* why) { return invalid_arg(who, (tag + field + why).c_str()); };
        if (d.width < 1) return refuse("width", " < 1");
        if (d.pad_after < 0 || d.pad_after > 3) return refuse("pad_after", " outside 0..3");
        const long long rows_dst = d.use_map ? x->rows_new : 1, rows_src = d.use_map ? x->rows_old : 1, rows_app = d.use_map ? x->rows_app : 0;
        if (rows_dst * d.width >= (1LL << 31) || rows_src * d.width >= (1LL << 31) || rows_app * d.width >= (1LL << 31))
            return set_last_error(MOSS_ERR_UNSUPPORTED, (std::string(who) + ": " + tag + "width: rows * width >= 2^31").c_str());
        const size_t n_src = (size_t)(rows_src * d.width), n_app = (size_t)(rows_app * d.width), n_body = (size_t)(rows_dst * d.width);
        if (!d.dst && n_body + d.pad_after > 0) return refuse("dst", " is null");
        if (!d.src && n_src > 0 && n_body > 0) return refuse("src", " is null");
        if (!d.app && n_app > 0 && n_body > 0) return refuse("app", " is null");
        const bool moments = d.src_m || d.src_v || d.dst_m || d.dst_v;           // (given together or not at all)
        if (moments) {
            if (!d.dst_m) return refuse("dst_m", " is null although another moment pointer is given");
            if (!d.dst_v) return refuse("dst_v", " is null although another moment pointer is given");
            if (!d.src_m && n_src > 0 && n_body > 0) return refuse("src_m", " is null although another moment pointer is given");
            if (!d.src_v && n_src > 0 && n_body > 0) return refuse("src_v", " is null although another moment pointer is given");
        }
        sources.push_back(bytes(d.src, d.src ? n_src : 0, tag + "src"));
        sources.push_back(bytes(d.app, d.app ? n_app : 0, tag + "app"));
        dests.push_back(bytes(d.dst, n_body + d.pad_after, tag + "dst"));
        if (moments) {
            sources.push_back(bytes(d.src_m, d.src_m ? n_src : 0, tag + "src_m"));
            sources.push_back(bytes(d.src_v, d.src_v ? n_src : 0, tag + "src_v"));
            dests.push_back(bytes(d.dst_m, n_body + d.pad_after, tag + "dst_m"));
            dests.push_back(bytes(d.dst_v, n_body + d.pad_after, tag + "dst_v"));
        }
        RelayoutTensor& t = a.t[i];
        t.src = d.src; t.src_m = d.src_m; t.src_v = d.src_v; t.app = d.app;
        t.dst = d.dst; t.dst_m = d.dst_m; t.dst_v = d.dst_v;
        t.width = d.width; t.use_map = d.use_map ? 1 : 0;
        t.n_body = (unsigned)n_body; t.n_total = (unsigned)(n_body + d.pad_after);
        a.block_start[i] = (int)grid;
        grid += ((long long)t.n_total + RW_TILE - 1) / RW_TILE;
    }
    if (grid > 0x7fffffffLL) return set_last_error(MOSS_ERR_UNSUPPORTED, (std::string(who) + ": num_tensors: the grid exceeds 2^31 workgroups").c_str());
    for (int i = x->num_tensors; i <= MOSS_ROWS_MAX_TENSORS; i++) a.block_start[i] = (int)grid;
    for (size_t i = 0; i < dests.size(); i++) {
        for (const Range& s : sources)
            if (overlap(dests[i], s)) return invalid_arg(who, (dests[i].name + " overlaps " + s.name).c_str());
        for (size_t j = 0; j < i; j++)
            if (overlap(dests[i], dests[j])) return invalid_arg(who, (dests[i].name + " overlaps " + dests[j].name).c_str());
    }
    if (grid == 0) return 0;
    hipLaunchKernelGGL(rows_relayout_kernel, dim3((unsigned)grid), dim3(RW_BLOCK), 0, (hipStream_t)stream, a);
    return launch_status(who);
}
