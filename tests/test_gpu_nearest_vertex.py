"""The nearest-template-vertex op on the GPU (``moss_amd.knn_cuda.TemplateIndex``, csrc/nearest_vertex.hip): ids and distances are
those of the brute-force query ``knn(ref, q, 1, "brute")`` BIT FOR BIT -- the op adds an index, not arithmetic, so every comparison
here is ``torch.equal`` -- and its three users (``lbs.coarse_deform_c2source``, ``densify.densify_and_prune_fused``; ``MossStep`` has a
file of its own) return what they returned without it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_moss_step import _release_device_memory  # noqa: F401  (autouse: the module leaves the device as it found it)

pytestmark = pytest.mark.gpu

VS = (1, 2, 63, 64, 65, 129, 6890, 20000)            # one vertex; the block edges; two and three blocks; MOSS's template; 313 blocks
PS = (1, 63, 64, 65, 1000)                           # fewer queries than a workgroup's waves ... more than one workgroup


def _body(n, seed, spread=0.02):
    """Body-like points: a jittered tube (the generator of tests/test_gpu_ops.py's cell-grid tests)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g) * 1.7
    ang = torch.rand(n, generator=g) * 6.2831853
    rad = 0.1 + 0.1 * torch.rand(n, generator=g)
    return (torch.stack([rad * torch.cos(ang), t, rad * torch.sin(ang)], 1) + spread * torch.randn(n, 3, generator=g)).float()


def _brute(ref, q):
    from moss_amd.knn_cuda import knn
    d, i = knn(ref[None], q[None], 1, "brute")
    return i.reshape(-1), d.reshape(-1)


def _same_as_brute(ref, q, what=""):
    from moss_amd.knn_cuda import TemplateIndex
    index = TemplateIndex(ref)
    ids, dist = index.query(q, want_dist=True)
    i0, d0 = _brute(ref, q)
    assert ids.dtype == torch.int64 and dist.dtype == torch.float32 and ids.shape == dist.shape == (q.shape[0],)
    assert torch.equal(ids, i0), what
    assert torch.equal(dist, d0), what
    assert torch.equal(index.query(q), i0), what                                     # (without the distance)
    return index, ids, dist


@pytest.mark.parametrize("V", VS)
def test_ids_and_distances_equal_brute_force(gpu, hip_lib, V):
    from moss_amd.knn_cuda import TemplateIndex
    ref = _body(V, 10 + V).to(gpu)
    index = TemplateIndex(ref[None])                                                 # ((1, V, 3) is taken too)
    assert index.V == V
    for P in PS:
        q = _body(P, 1000 + P).to(gpu)
        ids, dist = index.query(q, want_dist=True)
        i0, d0 = _brute(ref, q)
        assert torch.equal(ids, i0) and torch.equal(dist, d0), (V, P)
        assert torch.equal(index.query(q), i0), (V, P)
        assert int(ids.min()) >= 0 and int(ids.max()) < V


def test_matches_the_exhaustive_oracle(gpu, hip_lib):
    from moss_amd.knn_cuda import TemplateIndex
    from oracle import oracle
    ref, q = _body(5000, 3), _body(4000, 4)
    ids, dist = TemplateIndex(ref.to(gpu)).query(q.to(gpu), want_dist=True)
    d_ref, i_ref = oracle.knn_exhaustive(ref.numpy(), q.numpy(), 1)
    assert np.array_equal(ids.cpu().numpy(), i_ref.reshape(-1))
    np.testing.assert_array_equal(dist.cpu().numpy(), d_ref.reshape(-1))


def test_ties_go_to_the_lowest_vertex_index(gpu, hip_lib):
    g = torch.Generator().manual_seed(5)
    base = torch.rand(1500, 3, generator=g)
    ref = torch.cat([base, base[:700]]).to(gpu)
    q = torch.cat([base[:900], base[:200] + 0.01]).to(gpu)
    _, ids, dist = _same_as_brute(ref, q, "cat(base, base[:700])")
    assert torch.equal(ids[:900].cpu(), torch.arange(900)) and float(dist[:900].abs().max()) == 0.0
    # an integer lattice without its centre: six vertices at distance 1 from the centre, in every order
    r = torch.arange(-2, 3, dtype=torch.float32)
    lattice = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[lattice.abs().sum(1) > 0]
    for seed in range(3):
        perm = torch.randperm(lattice.shape[0], generator=torch.Generator().manual_seed(seed))
        verts = lattice[perm]
        q = torch.cat([torch.zeros(1, 3), 0.5 * torch.ones(1, 3), verts[:20]]).to(gpu)      # (0.5, 0.5, 0.5): eight at the same distance
        _, ids, dist = _same_as_brute(verts.to(gpu), q, f"lattice {seed}")
        assert int(ids[0]) == int(torch.nonzero(verts.abs().sum(1) == 1)[:, 0].min()) and float(dist[0]) == 1.0
    # the same triplicated set under three permutations: the lowest of the three tied positions
    base = _body(300, 8)
    trip = torch.cat([base, base, base])
    for seed in range(3):
        perm = torch.randperm(900, generator=torch.Generator().manual_seed(40 + seed))
        where = torch.empty(900, dtype=torch.int64)
        where[perm] = torch.arange(900)                                              # trip[j] sits at where[j] of trip[perm]
        _, ids, dist = _same_as_brute(trip[perm].to(gpu), base.to(gpu), f"permutation {seed}")
        assert torch.equal(ids.cpu(), where.reshape(3, 300).min(0).values) and float(dist.max()) == 0.0


def test_degenerate_sets_and_far_queries(gpu, hip_lib):
    g = torch.Generator().manual_seed(6)
    flat = torch.rand(1500, 3, generator=g)
    flat[:, 2] = 0.25
    far = torch.tensor([[1e4, 0.0, 0.0], [-1e4, 1e4, 0.25], [0.5, 0.5, -1e4], [1e4, 1e4, 1e4], [5.0, -3.0, 2.0]])
    q = torch.cat([flat[:300], torch.rand(300, 3, generator=g), far]).to(gpu)
    _, ids, dist = _same_as_brute(flat.to(gpu), q, "coplanar")
    assert float(dist[:300].max()) == 0.0 and float(dist[-5:].min()) > 3.0           # on a vertex: exactly 0
    same = torch.full((3000, 3), 0.5).to(gpu)
    _, ids, _ = _same_as_brute(same, q, "identical")
    assert not bool(ids.any())
    _same_as_brute(_body(6890, 9).to(gpu), torch.cat([_body(500, 10) * 1e4, far]).to(gpu), "10^4 away")


def test_non_finite_queries_get_minus_one_and_leave_their_neighbours_alone(gpu, hip_lib):
    ref = _body(6890, 11).to(gpu)
    q = _body(200, 12).to(gpu)
    index, ids0, dist0 = _same_as_brute(ref, q)
    bad = q.clone()
    bad[7, 0], bad[64, 1], bad[65, 2], bad[199] = float("nan"), float("inf"), float("-inf"), float("nan")
    ids, dist = index.query(bad, want_dist=True)
    i0, d0 = _brute(ref, bad)
    assert torch.equal(ids, i0) and torch.equal(dist, d0)
    rows = torch.tensor([7, 64, 65, 199], device=gpu)
    keep = torch.ones(200, dtype=torch.bool, device=gpu)
    keep[rows] = False
    assert bool((ids[rows] == -1).all()) and bool(torch.isinf(dist[rows]).all()) and bool((dist[rows] > 0).all())
    assert torch.equal(ids[keep], ids0[keep]) and torch.equal(dist[keep], dist0[keep])


def test_no_queries_and_a_snapshot_of_the_vertices(gpu, hip_lib):
    from moss_amd.knn_cuda import TemplateIndex
    ref = _body(700, 13).to(gpu)
    q = _body(300, 14).to(gpu)
    i0, d0 = _brute(ref, q)
    index = TemplateIndex(ref)
    ids, dist = index.query(torch.zeros(0, 3, device=gpu), want_dist=True)
    assert ids.shape == (0,) and dist.shape == (0,) and ids.dtype == torch.int64
    ref.zero_()                                                                      # the index holds its own copy
    ids, dist = index.query(q, want_dist=True)
    assert torch.equal(ids, i0) and torch.equal(dist, d0)
    with pytest.raises(RuntimeError, match="expected points"):
        index.query(q.cpu())


def test_c_abi_null_distance_and_guard_elements(gpu, hip_lib):
    from moss_amd import _lib
    from moss_amd.knn_cuda import TemplateIndex
    ref = _body(6890, 15).to(gpu)
    index = TemplateIndex(ref)
    for P in (1, 63, 257):
        q = _body(P, 16 + P).to(gpu)
        i0, d0 = _brute(ref, q)
        ids = torch.full((P + 8,), -77, dtype=torch.int64, device=gpu)
        dist = torch.full((P + 8,), -5.0, device=gpu)
        _lib.call("moss_nearest_vertex_query", gpu, index.V, P, index._index.data_ptr(), index._bytes, q.data_ptr(), ids.data_ptr(), dist.data_ptr())
        assert torch.equal(ids[:P], i0) and torch.equal(dist[:P], d0)
        assert bool((ids[P:] == -77).all()) and bool((dist[P:] == -5.0).all())
        ids2 = torch.full((P + 8,), -77, dtype=torch.int64, device=gpu)
        _lib.call("moss_nearest_vertex_query", gpu, index.V, P, index._index.data_ptr(), index._bytes, q.data_ptr(), ids2.data_ptr(), None)
        assert torch.equal(ids2, ids)


def test_query_captured_and_replayed_on_new_points(gpu, hip_lib):
    from moss_amd.knn_cuda import TemplateIndex
    ref = _body(6890, 17).to(gpu)
    index = TemplateIndex(ref)
    P = 3000
    pts = _body(P, 18).to(gpu)
    ids = torch.empty(P, dtype=torch.int64, device=gpu)
    dist = torch.empty(P, dtype=torch.float32, device=gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        index.query(pts, want_dist=True, ids=ids, dist=dist)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        index.query(pts, want_dist=True, ids=ids, dist=dist)
    for k in range(3):
        new = _body(P, 19 + k, spread=0.02 * (k + 1)).to(gpu)
        pts.copy_(new)
        graph.replay()
        i1, d1 = index.query(new, want_dist=True)
        assert torch.equal(ids, i1) and torch.equal(dist, d1), k
    del graph


def test_no_host_sync(gpu, hip_lib):
    """Build and query run clean under torch.cuda.set_sync_debug_mode("error") (as tests/test_gpu_lbs.py::test_no_host_sync)."""
    from moss_amd.knn_cuda import TemplateIndex
    ref, q = _body(6890, 21).to(gpu), _body(4000, 22).to(gpu)
    TemplateIndex(ref).query(q, want_dist=True)                                      # (allocator warm-up outside the checked window)
    torch.cuda.synchronize(gpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids, dist = TemplateIndex(ref).query(q, want_dist=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize(gpu)
    i0, d0 = _brute(ref, q)
    assert torch.equal(ids, i0) and torch.equal(dist, d0)


def test_coarse_deform_c2source_is_unchanged_by_a_template_index(gpu, hip_lib):
    from moss_amd import lbs as mlbs
    from moss_amd.knn_cuda import KNN, TemplateIndex
    P, V, J = 3000, 6890, 24
    body = mlbs.synthetic_body_model(V, J, device=gpu)
    params, t_params = mlbs.synthetic_frame(3, J, device=gpu), mlbs.synthetic_frame(0, J, big_pose=True, device=gpu)
    t_vertices = body["v_template"][None].clone()
    g = torch.Generator().manual_seed(23)
    x0 = (body["v_template"].cpu()[torch.randint(0, V, (P,), generator=g)] + 0.01 * torch.randn(P, 3, generator=g)).to(gpu)
    L0 = torch.randn(1, P, J, generator=g).to(gpu)
    cot = [torch.randn(*s, generator=g).to(gpu) for s in ((1, P, 3), (1, P, 3), (1, P, 3, 3), (1, P, 3))]
    results = []
    for with_index in (False, True):
        model = SimpleNamespace(SMPL_NEUTRAL=body, knn=KNN(k=1, transpose_mode=True))
        if with_index:
            model.template_index = TemplateIndex(t_vertices)
        x, L = x0.clone().requires_grad_(True), L0.clone().requires_grad_(True)
        out = mlbs.coarse_deform_c2source(model, x[None], params, t_params, t_vertices, lbs_weights=L, return_transl=True)
        loss = sum((out[k] * c).sum() for k, c in zip((0, 1, 3, 4), cot))
        results.append((out, torch.autograd.grad(loss, [x, L])))
    (o0, g0), (o1, g1) = results
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1]) and bool(g0[0].any()) and bool(g0[1].any())
    model.template_index = TemplateIndex(t_vertices[0, :100])
    with pytest.raises(ValueError, match="template_index holds 100 vertices"):
        mlbs.coarse_deform_c2source(model, x0[None], params, t_params, t_vertices)
    model.template_index = None                                                      # (None: the model's knn again)
    assert torch.equal(mlbs.coarse_deform_c2source(model, x0[None], params, t_params, t_vertices, lbs_weights=L0)[1], o0[1].detach())


def test_densify_and_prune_fused_is_unchanged_by_a_template_index(gpu, hip_lib):
    from moss_amd import densify as D
    from moss_amd.knn_cuda import TemplateIndex
    from tests.golden import make_golden_densify as gold
    from tests.test_gpu_densify_decision import _driver_set
    case = list(gold.CASES)[0]
    g = gold.golden_inputs(case)
    tv = g["t_vertices"].to(gpu)
    runs = []
    for with_index in (False, True):
        pc, _, opt = _driver_set(g, gpu)
        stats = D.DensifyStats(gold.P, device=gpu)
        stats.xyz_gradient_accum.copy_(g["accum"].to(gpu)); stats.denom.copy_(g["denom"].to(gpu)); stats.max_radii2D.copy_(g["max_radii2D"].to(gpu))
        noise = iter([g["noise_clone"], g["noise_split"]])
        rep = D.densify_and_prune_fused(pc, opt, stats, g["joint_F"].to(gpu), g["lbs_weights"].to(gpu), gold.MAX_GRAD, gold.MIN_OPACITY, gold.EXTENT,
                                        gold.SCREEN[case], tv, kl_threshold=gold.KL_THRESHOLD, surface_mask=g["surface_mask"].to(gpu),
                                        generator=lambda n: next(noise)[:n], percent_dense=gold.PERCENT_DENSE,
                                        template_index=TemplateIndex(tv) if with_index else None)
        runs.append((rep, [p.detach().clone() for p in (pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation)]))
    (r0, p0), (r1, p1) = runs
    assert r0 == r1, (r0, r1)
    from moss_amd.knn_cuda import knn
    assert torch.equal(TemplateIndex(tv).query(p0[0], want_dist=True)[1], knn(tv.reshape(1, -1, 3), p0[0][None], 1)[0].reshape(-1))
    for a, b in zip(p0, p1):
        assert a.shape == b.shape and torch.equal(a, b)
