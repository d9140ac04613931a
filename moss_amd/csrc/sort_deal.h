// sort_deal.h -- which sort chunk a workgroup of chunk_sort_kernel takes on its turn (binning.hip, the self-scan path).
// Host + device, so that the mapping can be checked on a CPU (tests/test_sort_deal_cpu.py).
//
// A tile of n keys has ceil(n / CHUNK) chunks, numbered in tile order; all but its LAST chunk are full.  A chunk's network runs to its
// padded size (64, 128, ... CHUNK keys): that is its size CLASS, 0 .. TOP.  Turn r of the kernel (workgroup wg takes the turns wg,
// wg + grid, ...) sorts the r-th chunk of this order: classes from the largest to the smallest, chunk index ascending inside a class.
// The workgroups that are dispatched first -- one per CU -- so get the frame's full chunks, and the ones that have to share a CU the
// smallest, whose networks are a third as long and whose idle waves leave at once.
//
// What the workgroup needs for it is cheap because only a tile's LAST chunk can be of a class below TOP ("a small tile"): with
//   small_total[k]   tiles of the frame whose last chunk is of class k < TOP,
//   before(tile)     k < TOP: tiles in front of this one whose last chunk is of class k; k = TOP: ... of ANY class below TOP
// the r-th chunk is found by every tile testing itself (sort_deal_claim): the chunks of class TOP in front of a tile are its chunk
// base minus the small tiles in front of it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SORT_DEAL_HD __host__ __device__ __forceinline__
#else
#define SORT_DEAL_HD inline
#endif

namespace moss {
namespace sort_deal {

constexpr uint32_t CHUNK = 1024u, MIN_PAD = 64u;             // keys of a full chunk; the smallest padded size (binning.hip asserts both)
constexpr uint32_t TOP = 4u;                                 // class of a chunk padded to CHUNK keys: log2(CHUNK / MIN_PAD)
constexpr uint32_t NONE = 0xffffffffu;
static_assert((MIN_PAD << TOP) == CHUNK, "TOP = log2(CHUNK / MIN_PAD)");

// class of a chunk of n keys (1 .. CHUNK): log2 of its padded size over MIN_PAD
SORT_DEAL_HD uint32_t class_of(uint32_t n)
{
    return n <= MIN_PAD ? 0u : (uint32_t)(32 - __builtin_clz(n - 1u)) - (uint32_t)(31 - __builtin_clz(MIN_PAD));
}

// class of the last chunk of a tile of n keys; an empty tile has no chunk: NONE
SORT_DEAL_HD uint32_t last_class(uint32_t n)
{
    return n ? class_of(n - ((n - 1u) / CHUNK) * CHUNK) : NONE;
}

// turn r (< n_chunks) -> the class k of the chunk sorted on it and q, the chunk's index among the frame's chunks of that class
SORT_DEAL_HD void turn_class(uint32_t r, uint32_t n_chunks, const uint32_t (&small_total)[TOP], uint32_t& k, uint32_t& q)
{
    uint32_t small = 0u;
    for (uint32_t i = 0; i < TOP; i++) small += small_total[i];
    uint32_t base = n_chunks - small;                        // chunks of class TOP come first
    k = TOP; q = r;
    for (uint32_t i = TOP; i-- > 0u;) {
        if (r >= base) { k = i; q = r - base; }
        base += small_total[i];
    }
}

// The chunk that a tile of n keys with chunk base cb contributes as the q-th chunk of class k, or NONE.  lc = last_class(n) (the kernel
// keeps it packed in a register); `before`: see above.
SORT_DEAL_HD uint32_t claim(uint32_t k, uint32_t q, uint32_t n, uint32_t lc, uint32_t cb, uint32_t before)
{
    const uint32_t nch = (n + CHUNK - 1u) / CHUNK;
    if (k < TOP) return (lc == k && before == q) ? cb + nch - 1u : NONE;
    const uint32_t first = cb - before;                      // chunks of class TOP in front of this tile
    const uint32_t mine = nch - (lc < TOP ? 1u : 0u);        // (lc == NONE: an empty tile, nch = 0)
    return (q >= first && q - first < mine) ? cb + (q - first) : NONE;
}

}  // namespace sort_deal
}  // namespace moss
