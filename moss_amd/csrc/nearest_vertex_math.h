// nearest_vertex_math.h -- the float32 arithmetic of the nearest-template-vertex op (nearest_vertex.hip): the squared distance, the
// order of candidates, the two bounds of a block's box, the Morton key of the build.  Host + device, so that the pruning can be
// checked on a CPU against an exhaustive search (tests/test_nearest_vertex_cpu.py).
//
// WHY THE BOUNDS ARE CONSERVATIVE IN FLOAT32, WITH NO ALLOWANCE.  Every operation below is a correctly rounded IEEE operation (this
// header and its users are compiled without FMA contraction), and a correctly rounded operation is MONOTONE: a <= b implies
// fl(a - c) <= fl(b - c), and for non-negative operands fl(a * a) <= fl(b * b) and fl(a + c) <= fl(b + c).  A box holds the exact
// minimum and maximum of its vertices' coordinates (min / max do not round).  For a vertex v of the box and a query q, per axis:
//   q < lo:        0 < lo - q <= v - q, so  e = fl(lo - q) <= fl(v - q) = |dx|
//   q > hi:        0 < q - hi <= q - v, so  e = fl(q - hi) <= fl(q - v) = |fl(v - q)| = |dx|   (rounding is symmetric in sign)
//   lo <= q <= hi: e = 0 <= |dx|
// and |dx| <= f = max(|fl(lo - q)|, |fl(hi - q)|), because v - q lies between lo - q and hi - q.  dist2() and the two bounds then
// square and add IN THE SAME ORDER -- (x*x + y*y) + z*z -- so monotonicity carries through every rounding:
//   box_lower_bound(box, q) <= dist2(v, q) <= box_upper_bound(box, q)      as float32 values, exactly, for every v in the box.
// The allowance for "rounding of the bound itself" is therefore zero, and the search skips a block only when its lower bound is
// STRICTLY greater than the best distance so far: a block that could hold an equal distance (a tie, which goes to the lower vertex
// index whatever the visit order) is always evaluated.  Infinite coordinates keep all of this (inf arithmetic is monotone too); a
// NaN vertex coordinate never enters a box (fminf / fmaxf drop it) and never wins (NaN compares false); a non-finite QUERY is
// answered before any bound is formed.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define NV_MATH_HD __host__ __device__ __forceinline__
#else
#define NV_MATH_HD inline
#endif

namespace moss {
namespace nearest_vertex {

constexpr int BLOCK = 64;                 // vertices per block: one per lane of a wave
constexpr int MAX_V = 65536;              // the vertex index rides in 16 bits of the build's sort key
constexpr int MORTON_BITS = 10;           // per axis

NV_MATH_HD int blocks_for(int V) { return (V + BLOCK - 1) / BLOCK; }

// the brute-force kernel's expression (knn_query.hip: dx = r.x - qx, ..., d = dx * dx + dy * dy + dz * dz), bit for bit
NV_MATH_HD float dist2(float vx, float vy, float vz, float qx, float qy, float qz)
{
#pragma clang fp contract(off)
    const float dx = vx - qx, dy = vy - qy, dz = vz - qz;
    return dx * dx + dy * dy + dz * dz;
}

// (d, id) is a better answer than (bd, bi): strictly closer, or as close with the lower vertex index.  The search starts from
// (+inf, -1): nothing is "as close with a lower index" than that, so a vertex at distance +inf or NaN never replaces it.
NV_MATH_HD bool closer(float d, int id, float bd, int bi) { return d < bd || (d == bd && id < bi); }

// squared distance from q to the box [lo, hi]: never above dist2 of a vertex inside (see the top of the file)
NV_MATH_HD float box_lower_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz)
{
#pragma clang fp contract(off)
    const float ex = fmaxf(fmaxf(lox - qx, qx - hix), 0.0f);
    const float ey = fmaxf(fmaxf(loy - qy, qy - hiy), 0.0f);
    const float ez = fmaxf(fmaxf(loz - qz, qz - hiz), 0.0f);
    return ex * ex + ey * ey + ez * ez;
}

// squared distance from q to the farthest corner of the box: never below dist2 of a vertex inside
NV_MATH_HD float box_upper_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz)
{
#pragma clang fp contract(off)
    const float fx = fmaxf(fabsf(lox - qx), fabsf(hix - qx));
    const float fy = fmaxf(fabsf(loy - qy), fabsf(hiy - qy));
    const float fz = fmaxf(fabsf(loz - qz), fabsf(hiz - qz));
    return fx * fx + fy * fy + fz * fz;
}

// A block is skipped iff this holds: strictly, never on equality.  (NaN `best` cannot occur: it starts at +inf and only falls.)
NV_MATH_HD bool can_skip(float lower_bound, float best) { return lower_bound > best; }

// ---- the build's sort key: position along a Morton curve of the bounding box, then the vertex index (which makes keys unique).
// The order only decides which vertices share a block, i.e. how tight the boxes are -- never the answer.
NV_MATH_HD uint32_t spread3(uint32_t v)                       // 10 bits -> every third bit
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// cell of x along one axis: CUBIC cells (the same size on every axis, 2^MORTON_BITS of them along the box's longest edge) -- cells
// stretched to the box's proportions give blocks stretched the same way, and a body is five times as tall as it is deep
NV_MATH_HD uint32_t morton_cell(float x, float lo, float inv)
{
    const float c = fminf(fmaxf((x - lo) * inv, 0.0f), (float)((1 << MORTON_BITS) - 1));     // NaN -> 0
    return (uint32_t)c;
}
NV_MATH_HD uint64_t morton_key(float x, float y, float z, const float* lo, const float* hi, uint32_t index)
{
    const float ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    const float inv = ext > 0.0f && ext < INFINITY ? (float)(1 << MORTON_BITS) / ext : 0.0f;
    const uint32_t m = spread3(morton_cell(x, lo[0], inv)) | (spread3(morton_cell(y, lo[1], inv)) << 1) | (spread3(morton_cell(z, lo[2], inv)) << 2);
    return ((uint64_t)m << 32) | index;
}

}  // namespace nearest_vertex
}  // namespace moss
