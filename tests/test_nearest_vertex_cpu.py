"""CPU tests of the nearest-template-vertex op (csrc/nearest_vertex.hip): the arithmetic it shares with the host
(csrc/nearest_vertex_math.h), its C ABI and its Python class.

A small host program includes the header the kernels include, builds the index as the build kernels do (bounding box, Morton keys,
sort, blocks of 64, exact boxes), runs the query kernel's search -- the nearest box first, then every block whose lower bound is not
strictly above the best distance, candidates ordered by ``closer`` -- and an exhaustive search written independently of the header's
order (ascending index, strictly closer wins: the brute-force kernel's loop) over the same ``dist2``.  It also checks, for every
query and every box, ``lower bound <= dist2(v) <= upper bound`` for every vertex of the box.  Queries: the ones given (on vertices,
around the set, 10^4 away) plus, added by the program, the face centres and the two extreme corners of every box."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "nearest_vertex_math.h"
using namespace moss::nearest_vertex;
struct Box { float lo[3], hi[3]; };
// stdin, per case: int32 V, Q; float32 verts[3V], queries[3Q].
// stdout, per case: int32 n (queries, with the box queries), NB, sandwich violations; then per query int32 {pruned id, exhaustive id, blocks evaluated}.
int main()
{
    int32_t V, Q;
    while (fread(&V, 4, 1, stdin) == 1 && fread(&Q, 4, 1, stdin) == 1) {
        std::vector<float> v(3 * (size_t)V), q(3 * (size_t)Q);
        if (fread(v.data(), 4, v.size(), stdin) != v.size() || fread(q.data(), 4, q.size(), stdin) != q.size()) return 2;
        // ---- the index, as nv_keys_kernel / nv_rank_scatter_kernel / nv_boxes_kernel build it
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int i = 0; i < V; i++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], v[3 * i + k]); hi[k] = fmaxf(hi[k], v[3 * i + k]); }
        std::vector<uint64_t> keys(V);
        for (int i = 0; i < V; i++) keys[i] = morton_key(v[3 * i], v[3 * i + 1], v[3 * i + 2], lo, hi, (uint32_t)i);
        std::sort(keys.begin(), keys.end());
        const int NB = blocks_for(V);
        std::vector<int> order(V);
        for (int i = 0; i < V; i++) order[i] = (int)(keys[i] & 0xffffffffu);
        std::vector<Box> box(NB);
        for (int b = 0; b < NB; b++) {
            for (int k = 0; k < 3; k++) { box[b].lo[k] = INFINITY; box[b].hi[k] = -INFINITY; }
            for (int s = b * BLOCK; s < std::min(V, (b + 1) * BLOCK); s++)
                for (int k = 0; k < 3; k++) { const float x = v[3 * order[s] + k]; box[b].lo[k] = fminf(box[b].lo[k], x); box[b].hi[k] = fmaxf(box[b].hi[k], x); }
        }
        // ---- more queries: on every box's faces and at its two extreme corners
        for (int b = 0; b < NB; b++) {
            const float* l = box[b].lo; const float* h = box[b].hi;
            const float m[3] = { 0.5f * (l[0] + h[0]), 0.5f * (l[1] + h[1]), 0.5f * (l[2] + h[2]) };
            for (int k = 0; k < 3; k++) for (int side = 0; side < 2; side++) { float p[3] = { m[0], m[1], m[2] }; p[k] = side ? h[k] : l[k]; q.insert(q.end(), p, p + 3); }
            q.insert(q.end(), l, l + 3); q.insert(q.end(), h, h + 3);
        }
        const int32_t n = (int32_t)(q.size() / 3);
        int32_t bad = 0;
        std::vector<int32_t> out;
        for (int j = 0; j < n; j++) {
            const float qx = q[3 * j], qy = q[3 * j + 1], qz = q[3 * j + 2];
            auto lower = [&](int b) { return box_lower_bound(box[b].lo[0], box[b].lo[1], box[b].lo[2], box[b].hi[0], box[b].hi[1], box[b].hi[2], qx, qy, qz); };
            // the sandwich, for every vertex of every box
            for (int b = 0; b < NB; b++) {
                const float lb = lower(b), ub = box_upper_bound(box[b].lo[0], box[b].lo[1], box[b].lo[2], box[b].hi[0], box[b].hi[1], box[b].hi[2], qx, qy, qz);
                for (int s = b * BLOCK; s < std::min(V, (b + 1) * BLOCK); s++) {
                    const int i = order[s];
                    const float d = dist2(v[3 * i], v[3 * i + 1], v[3 * i + 2], qx, qy, qz);
                    bad += !(lb <= d && d <= ub);
                }
            }
            // the pruned search, as nv_query_kernel runs it
            float bd = INFINITY; int bi = -1, evaluated = 0;
            auto eval = [&](int b) {
                evaluated++;
                for (int s = b * BLOCK; s < std::min(V, (b + 1) * BLOCK); s++) {
                    const int i = order[s];
                    const float d = dist2(v[3 * i], v[3 * i + 1], v[3 * i + 2], qx, qy, qz);
                    if (closer(d, i, bd, bi)) { bd = d; bi = i; }
                }
            };
            int first = 0; float mlb = INFINITY;
            for (int b = 0; b < NB; b++) { const float lb = lower(b); if (lb < mlb) { mlb = lb; first = b; } }
            eval(first);
            for (int b = 0; b < NB; b++) if (b != first && !can_skip(lower(b), bd)) eval(b);
            // the exhaustive search: the brute-force kernel's loop
            float ed = INFINITY; int ei = -1;
            for (int i = 0; i < V; i++) {
                const float dx = v[3 * i] - qx, dy = v[3 * i + 1] - qy, dz = v[3 * i + 2] - qz;
                const float d = dx * dx + dy * dy + dz * dz;
                if (d < ed) { ed = d; ei = i; }
            }
            out.push_back(bi); out.push_back(ei); out.push_back(evaluated);
        }
        const int32_t nb = NB;
        fwrite(&n, 4, 1, stdout); fwrite(&nb, 4, 1, stdout); fwrite(&bad, 4, 1, stdout);
        fwrite(out.data(), 4, out.size(), stdout);
    }
    return 0;
}
"""


def _body(rng, n):
    """Points on a few thin limbs: a surface-like set, as the template is."""
    t = rng.random(n)
    limb = rng.integers(0, 5, n)
    axis = np.array([[0, 1, 0], [0.7, -0.7, 0], [-0.7, -0.7, 0], [1, 0.2, 0], [-1, 0.2, 0]], dtype=np.float64)[limb]
    phi = rng.random(n) * 2 * np.pi
    ring = 0.08 * np.stack([np.cos(phi), np.zeros(n), np.sin(phi)], 1)
    return (axis * t[:, None] * 0.8 + ring).astype(np.float32)


def _queries(rng, verts):
    V = len(verts)
    on = verts[rng.permutation(V)[:min(V, 40)]]
    near = (verts[rng.integers(0, V, 60)] + 0.03 * rng.normal(size=(60, 3))).astype(np.float32)
    far = np.array([[1e4, 0, 0], [-1e4, 1e4, 0], [0, 0, -1e4], [1e4, 1e4, 1e4]], dtype=np.float32)
    return np.concatenate([on, near, far]).astype(np.float32)


def _cases():
    rng = np.random.default_rng(20250117)
    cases = []
    for V in (1, 63, 64, 65, 700):
        cases.append((f"body{V}", _body(rng, V)))
    base = _body(rng, 500)
    cases.append(("duplicates", np.concatenate([base, base[:200]])))                   # V = 700: every tie is between ids i and 500 + i
    flat = _body(rng, 700); flat[:, 2] = 0.25
    cases.append(("coplanar", flat))
    cases.append(("identical", np.tile(np.array([[0.3, -0.2, 0.1]], dtype=np.float32), (65, 1))))
    g = np.arange(-2, 3)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lattice = lattice[np.abs(lattice).sum(1) > 0]                                      # 124 vertices, the centre left out
    cases.append(("lattice", lattice[rng.permutation(len(lattice))]))
    out = []
    for name, verts in cases:
        q = _queries(rng, verts)
        if name == "lattice":
            q = np.concatenate([np.zeros((1, 3), dtype=np.float32), q])                # query 0: six vertices at distance 1
        out.append((name, np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)))
    return out


@pytest.fixture(scope="module")
def searched(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearest_vertex")
    src, exe = d / "search.cpp", d / "search"
    src.write_text(DRIVER)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "moss_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    cases = _cases()
    blob = b"".join(np.array([len(v), len(q)], dtype=np.int32).tobytes() + v.tobytes() + q.tobytes() for _, v, q in cases)
    words = np.frombuffer(subprocess.run([str(exe)], input=blob, capture_output=True, check=True).stdout, dtype=np.int32)
    out, at = {}, 0
    for name, v, q in cases:
        n, nb, bad = (int(x) for x in words[at:at + 3])
        body = words[at + 3: at + 3 + 3 * n].reshape(n, 3)
        at += 3 + 3 * n
        out[name] = dict(verts=v, queries=q, n=n, NB=nb, bad=bad, pruned=body[:, 0], exhaustive=body[:, 1], evaluated=body[:, 2])
    assert at == len(words)
    return out


def test_pruned_search_returns_the_exhaustive_search_s_ids(searched):
    assert set(searched) == {"body1", "body63", "body64", "body65", "body700", "duplicates", "coplanar", "identical", "lattice"}
    for name, c in searched.items():
        assert c["NB"] == (len(c["verts"]) + 63) // 64 and c["n"] == len(c["queries"]) + 8 * c["NB"], name
        assert np.array_equal(c["pruned"], c["exhaustive"]), name
        assert c["exhaustive"].min() >= 0, name
        # the exhaustive ids against numpy (float64 is exact enough to decide everything but ties, which it must not break upwards)
        d = ((c["verts"][None].astype(np.float64) - c["queries"][:, None].astype(np.float64)) ** 2).sum(-1)
        ids = c["exhaustive"][:len(c["queries"])]
        assert np.all(d[np.arange(len(ids)), ids] <= d.min(1) * (1 + 1e-6) + 1e-12), name


def test_ties_go_to_the_lowest_index_whatever_the_visit_order(searched):
    c = searched["lattice"]
    v = c["verts"]
    six = np.nonzero(np.abs(v).sum(1) == 1)[0]
    assert len(six) == 6 and c["pruned"][0] == six.min()
    c = searched["duplicates"]
    assert np.all(c["pruned"][:40] < 500)                                  # queries on vertices: the copy at 500 + i never wins
    c = searched["identical"]
    assert np.all(c["pruned"] == 0)


def test_bounds_sandwich_every_vertex_of_every_box(searched):
    for name, c in searched.items():
        assert c["bad"] == 0, name


def test_pruning_prunes(searched):
    """Not a correctness property -- but a search that evaluates every block is the brute force."""
    c = searched["body700"]
    near = c["evaluated"][:100]
    assert c["NB"] == 11 and np.all(c["evaluated"] >= 1) and np.all(c["evaluated"] <= 11) and np.median(near) <= 4


def test_header_declares_the_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text)
    flat = re.sub(r"\s+", " ", text)
    assert "size_t moss_nearest_vertex_index_bytes(int V);" in flat
    assert "int moss_nearest_vertex_build(int V, const float* vertices, char* index, size_t index_bytes, void* stream);" in flat
    assert ("int moss_nearest_vertex_query(int V, int P, const char* index, size_t index_bytes, const float* points, long long* ids_out, "
            "float* dist_out /* may be NULL */, void* stream);") in flat
    assert "scene/gaussian_model.py:827" in text[text.index("The nearest reference of every query"):text.index("size_t moss_nearest_vertex_index_bytes")]
    assert hip_lib.moss_abi_version() == 7
    for name in ("moss_nearest_vertex_index_bytes", "moss_nearest_vertex_build", "moss_nearest_vertex_query"):
        assert hasattr(hip_lib, name)
    from moss_amd import build
    assert build.SOURCES["nearest_vertex.hip"] == ["-ffp-contract=off"]


def test_index_bytes_grow_with_the_vertex_count(hip_lib):
    f = hip_lib.moss_nearest_vertex_index_bytes
    assert f(0) == 0 and f(-5) == 0 and f(65537) == 0
    sizes = [f(V) for V in (1, 64, 65, 6890, 20000, 65536)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[3] < sizes[5]
    assert f(6890) >= 108 * 64 * 16 + 108 * 32                             # the padded vertices and the boxes


def test_bad_arguments_are_refused_before_any_launch(hip_lib):
    b, q, n = hip_lib.moss_nearest_vertex_build, hip_lib.moss_nearest_vertex_query, hip_lib.moss_nearest_vertex_index_bytes(100)
    fake = 4096                                                            # (never dereferenced: every call below is refused)
    assert b(0, fake, fake, n, None) == -1 and b"V outside" in hip_lib.moss_last_error()
    assert b(65537, fake, fake, 1 << 30, None) == -1
    assert b(100, None, fake, n, None) == -1 and b"null vertices" in hip_lib.moss_last_error()
    assert b(100, fake, None, n, None) == -1
    assert b(100, fake, fake, n - 1, None) == -1 and b"index" in hip_lib.moss_last_error()
    assert q(0, 5, fake, n, fake, fake, None, None) == -1
    assert q(65537, 5, fake, 1 << 30, fake, fake, None, None) == -1
    assert q(100, -1, fake, n, fake, fake, None, None) == -1
    assert q(100, 5, None, n, fake, fake, None, None) == -1
    assert q(100, 5, fake, n - 1, fake, fake, None, None) == -1
    assert q(100, 5, fake, n, None, fake, None, None) == -1
    assert q(100, 5, fake, n, fake, None, None, None) == -1 and b"moss_nearest_vertex_query" in hip_lib.moss_last_error()
    assert q(100, 0, fake, n, None, None, None, None) == 0                 # P = 0: nothing to do, nothing to read


def test_template_index_has_no_cpu_path(hip_lib):
    import torch
    from moss_amd.knn_cuda import TemplateIndex
    with pytest.raises(RuntimeError, match="no CPU path"):
        TemplateIndex(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="expected vertices"):
        TemplateIndex(torch.zeros(10, 2))
    with pytest.raises(RuntimeError, match="expected vertices"):
        TemplateIndex(torch.zeros(0, 3))
