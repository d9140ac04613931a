"""CPU test of the sort kernel's deal of chunks to workgroups (csrc/sort_deal.h: turn r of chunk_sort_kernel's self-scan path sorts
the r-th chunk by padded size class, largest class first, chunk index ascending inside a class).  A small host program includes the
header the kernel includes and plays the workgroup: per-class totals, the counts in front of every tile, then ``turn_class`` and
``claim`` -- by every tile for every turn, as the kernel's threads do (for the 8192-tile vectors: for every 16th turn or so, and for
the others by the tile that holds the chunk).  Checked here, independently of the header: every chunk is visited exactly once
whatever the grid, the classes never grow along the turns, and chunks of one class come in index order."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024
TILES = (1, 7, 1024, 1025, 8192)
COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000)
GRIDS = (1, 2, 255, 256, 511)
VECTORS = 200
MORE_COUNTS = (129, 256, 257, 512, 513, 1024 + 200, 2048 + 400)

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "sort_deal.h"
using namespace moss::sort_deal;
// stdin: words {T, n[0 .. T-1]} per vector.  stdout, per vector: n_chunks, mismatches, then per turn {chunk, class}.
int main()
{
    uint32_t T;
    while (fread(&T, 4, 1, stdin) == 1) {
        std::vector<uint32_t> n(T), cb(T), lc(T), before_top(T), before[TOP];
        if (fread(n.data(), 4, T, stdin) != T) return 2;
        uint32_t small_total[TOP] = {}, n_chunks = 0, small = 0;
        for (uint32_t k = 0; k < TOP; k++) before[k].resize(T);
        for (uint32_t t = 0; t < T; t++) {
            cb[t] = n_chunks; n_chunks += (n[t] + CHUNK - 1) / CHUNK;
            lc[t] = last_class(n[t]);
            before_top[t] = small;
            for (uint32_t k = 0; k < TOP; k++) before[k][t] = small_total[k];
            if (lc[t] < TOP) { small_total[lc[t]]++; small++; }
        }
        std::vector<uint32_t> chunk(n_chunks, NONE), cls(n_chunks, NONE);
        uint32_t bad = 0;
        const size_t stride = (size_t)n_chunks * T <= 3000000 ? 1 : ((size_t)n_chunks * T + 2999999) / 3000000;
        for (uint32_t r = 0; r < n_chunks; r++) {
            uint32_t k, q;
            turn_class(r, n_chunks, small_total, k, q);
            cls[r] = k;
            if (r % stride == 0) {                         // every tile asks, as the kernel's threads do
                uint32_t claims = 0;
                for (uint32_t t = 0; t < T; t++) {
                    const uint32_t c = claim(k, q, n[t], lc[t], cb[t], k < TOP ? before[k][t] : before_top[t]);
                    if (c != NONE) { claims++; chunk[r] = c; }
                }
                bad += claims != 1;
            }
        }
        if (stride != 1) {                                  // the other turns: the tiles that hold a chunk of the class ask
            for (uint32_t r = 0; r < n_chunks; r++) {
                if (r % stride == 0) continue;
                uint32_t k, q;
                turn_class(r, n_chunks, small_total, k, q);
                uint32_t lo = 0, hi = T;                    // the last tile with that many in front of it or fewer, and its neighbours
                const std::vector<uint32_t>& b = k < TOP ? before[k] : before_top;
                if (k < TOP) { while (hi - lo > 1) { const uint32_t m = (lo + hi) / 2; if (b[m] <= q) lo = m; else hi = m; } }
                else { while (hi - lo > 1) { const uint32_t m = (lo + hi) / 2; if (cb[m] - b[m] <= q) lo = m; else hi = m; } }
                uint32_t claims = 0;
                for (uint32_t t = lo >= 8 ? lo - 8 : 0; t < T && t <= lo + 8; t++) {
                    const uint32_t c = claim(k, q, n[t], lc[t], cb[t], b[t]);
                    if (c != NONE) { claims++; chunk[r] = c; }
                }
                bad += claims != 1;
            }
        }
        fwrite(&n_chunks, 4, 1, stdout); fwrite(&bad, 4, 1, stdout);
        for (uint32_t r = 0; r < n_chunks; r++) { fwrite(&chunk[r], 4, 1, stdout); fwrite(&cls[r], 4, 1, stdout); }
    }
    return 0;
}
"""


def _vectors():
    rng = np.random.default_rng(20240607)
    out = []
    for i in range(VECTORS):
        T = TILES[i % len(TILES)]
        # (every few vectors: only some of the values, so that classes are missing and totals are lopsided)
        pool = COUNTS if i % 3 else rng.choice(COUNTS, size=int(rng.integers(1, 4)), replace=False)
        out.append(rng.choice(pool, size=T).astype(np.uint32))
    out[0][:] = 0                                           # a frame that renders nothing
    # (those counts pad to 64, 128 or 1024 keys only: twenty more vectors whose last chunks also pad to 256 and 512)
    for i in range(20):
        out.append(rng.choice(COUNTS + MORE_COUNTS, size=TILES[i % len(TILES)]).astype(np.uint32))
    return out


@pytest.fixture(scope="module")
def dealt(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_deal")
    src, exe = d / "deal.cpp", d / "deal"
    src.write_text(DRIVER)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "moss_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    vecs = _vectors()
    blob = b"".join(np.concatenate(([len(v)], v)).astype(np.uint32).tobytes() for v in vecs)
    words = np.frombuffer(subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout, dtype=np.uint32)
    out, at = [], 0
    for v in vecs:
        n_chunks, bad = int(words[at]), int(words[at + 1])
        body = words[at + 2: at + 2 + 2 * n_chunks].reshape(-1, 2)
        at += 2 + 2 * n_chunks
        out.append((v, n_chunks, bad, body[:, 0].astype(np.int64), body[:, 1].astype(np.int64)))
    assert at == len(words)
    return out


def _chunk_classes(counts):
    """Padded size class of every chunk, in chunk order -- restated from the kernel's padding loop, not from the header."""
    cls = []
    for n in counts.tolist():
        for c in range((n + CHUNK - 1) // CHUNK):
            keys, npad, k = min(CHUNK, n - c * CHUNK), 64, 0
            while npad < keys:
                npad, k = npad * 2, k + 1
            cls.append(k)
    return np.asarray(cls, dtype=np.int64)


def test_every_chunk_is_visited_exactly_once_for_every_grid(dealt):
    for counts, n_chunks, bad, chunk, _ in dealt:
        assert n_chunks == int(((counts.astype(np.int64) + CHUNK - 1) // CHUNK).sum())
        assert bad == 0, "a turn that no tile, or more than one tile, claimed"
        for grid in GRIDS:
            visited = np.concatenate([chunk[wg::grid] for wg in range(grid)]) if n_chunks else chunk
            assert np.array_equal(np.sort(visited), np.arange(n_chunks)), (len(counts), grid)


def test_classes_never_grow_along_the_turns_and_a_class_is_in_chunk_order(dealt):
    seen = set()
    for counts, n_chunks, _, chunk, cls in dealt:
        want = _chunk_classes(counts)
        assert len(want) == n_chunks
        assert np.array_equal(cls, want[chunk]), "the class of a turn is the class of the chunk it sorts"
        assert np.all(np.diff(cls) <= 0)
        same = np.diff(cls) == 0
        assert np.all(np.diff(chunk)[same] > 0)
        seen.update(cls.tolist())
    assert seen == {0, 1, 2, 3, 4}
