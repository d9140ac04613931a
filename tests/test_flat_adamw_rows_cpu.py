"""``optim.FlatAdamWRows``: several ``FlatAdamW`` presented as one optimizer for row surgery -- what ``MossStep`` needs to carry a
densification event out on its two Gaussian optimizers.  On CPU tensors the group runs the members' torch restatement of the gather,
so everything here runs without a GPU; the one launch over all members is tests/test_gpu_moss_step_events.py's.

A twin comparison: the same five row tensors (widths 3, 48, 1, 3, 4; P = 37, so the flat sizes are no multiples of 4) and one tensor
that is not per-row, once under ONE ``FlatAdamW`` and once split 4 + (1 + the other tensor) under the group.  Every call of
``GaussianSet``'s surgery is applied to both; parameters and both moments must stay equal bit for bit -- the group adds no arithmetic.
(``FlatAdamW.step()`` has no CPU path: the two steps that make the moments non-zero are tests/test_surgery_cpu.py's torch restatement
of the update on the optimizer's own buffers.)"""
import pytest
import torch

from moss_amd import scenes
from tests.test_surgery_cpu import _adamw_flat_, _new_rows, _postfix_args

P0 = 37


def _row_params(pc):
    return [pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation]


def _twin(split, hip_lib):
    """(pc, the other tensor, optimizer for surgery, members).  ``split``: 4 + 1 under the group; else one FlatAdamW."""
    from moss_amd import dist as mdist
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.optim import FlatAdamW, FlatAdamWRows
    pc = GaussianSet(scenes.config1(P=P0, seed=5), sh_degree=3, device="cpu", unified_features=True)
    assert [int(p[0].numel()) for p in _row_params(pc)] == [3, 48, 1, 3, 4]
    other = torch.nn.Parameter(torch.arange(5, dtype=torch.float32) + 0.5)
    groups = {g["name"]: g for g in pc.param_groups()}
    g_other = {"params": [other], "lr": 2e-3, "name": "other"}
    kw = dict(eps=1e-15, capturable=True)
    four = ("features", "opacity", "scaling", "rotation")
    if split:
        a = FlatAdamW([groups[n] for n in four], mdist.GradBucket([groups[n]["params"][0] for n in four]), **kw)
        b = FlatAdamW([groups["xyz"], g_other], mdist.GradBucket([pc._xyz, other]), **kw)
        members = [a, b]
        opt = FlatAdamWRows(members)
        assert [id(p) for p in opt.bucket.params] == [id(p) for p in (pc._features, pc._opacity, pc._scaling, pc._rotation, pc._xyz, other)]
    else:
        names = ("xyz",) + four
        opt = FlatAdamW([groups[n] for n in names] + [g_other], mdist.GradBucket([groups[n]["params"][0] for n in names] + [other]), **kw)
        members = [opt]
    # two steps on random gradients, the same per PARAMETER in both twins (a generator per parameter)
    for t in (1, 2):
        for o in members:
            bk = o.bucket
            grad = torch.zeros(bk.n_params)
            for p, n, off in zip(bk.params, bk.sizes, bk.offsets):
                which = [id(q) for q in _row_params(pc) + [other]].index(id(p))
                grad[off:off + n] = torch.randn(n, generator=torch.Generator().manual_seed(100 * t + which))
            _adamw_flat_(o, grad, t)
    for k, o in enumerate(members):                          # a step counter and a learning-rate block to find unchanged later
        o.t = 2
        o.step_state.copy_(torch.arange(o.step_state.numel(), dtype=torch.int32) + 1000 * (k + 1))
    return pc, other, opt, members


def _views(pc, other, members):
    """{parameter name: (values, exp_avg, exp_avg_sq)} whichever optimizer holds it."""
    names = dict(zip(("xyz", "features", "opacity", "scaling", "rotation", "other"), _row_params(pc) + [other]))
    out = {}
    for name, p in names.items():
        for o in members:
            idx = {id(q): i for i, q in enumerate(o.bucket.params)}
            if id(p) in idx:
                out[name] = (p.data,) + tuple(o._moments_of(idx[id(p)]))
    assert len(out) == 6
    return out


def _assert_equal(one, two, rows, what, zeroed=()):
    va, vb = _views(one[0], one[1], one[3]), _views(two[0], two[1], two[3])
    for name in va:
        for a, b, part in zip(va[name], vb[name], ("values", "exp_avg", "exp_avg_sq")):
            assert a.shape == b.shape and torch.equal(a, b), (what, name, part)
        if name != "other":
            assert va[name][0].shape[0] == rows, (what, name)
        if name != "other" and name not in zeroed:
            assert bool(va[name][1].any()) and bool(va[name][2].any()), (what, name)     # (the comparison is not of zeros)
    for k, o in enumerate(two[3] + one[3]):
        bk = o.bucket
        for n, off, nxt in zip(bk.sizes, bk.offsets, list(bk.offsets[1:]) + [bk.n_params]):     # zeros in the alignment gaps
            for flat in (o.flat_params, o.exp_avg, o.exp_avg_sq):
                assert not bool(flat[off + n:nxt].any()), what
        for p, off in zip(bk.params, bk.offsets):
            assert p.grad is None and p.data_ptr() == o.flat_params[off:off + 1].data_ptr()
        assert o.n == bk.n_params == o.flat_params.numel() == o.exp_avg.numel() == o.exp_avg_sq.numel()
    for k, o in enumerate(two[3]):                           # every member's step counter and learning-rate block: bit for bit
        assert o.t == 2 and torch.equal(o.step_state, torch.arange(o.step_state.numel(), dtype=torch.int32) + 1000 * (k + 1)), what


def _six(d):
    return {"new_xyz": d["xyz"], "new_features_dc": d["f_dc"], "new_features_rest": d["f_rest"], "new_opacities": d["opacity"],
            "new_scaling": d["scaling"], "new_rotation": d["rotation"]}


def test_group_of_two_equals_one_flat_adamw_through_every_surgery_call(hip_lib):
    from moss_amd.densify import DensifyStats
    one, two = _twin(False, hip_lib), _twin(True, hip_lib)
    objs = [[id(p) for p in o.bucket.params] for o in two[3]]
    _assert_equal(one, two, P0, "after two steps")
    other_before = [x.clone() for x in _views(two[0], two[1], two[3])["other"]]
    lr_xyz = float(two[3][1].seg_lr[0])
    stats = []
    for _ in range(2):
        s = DensifyStats.__new__(DensifyStats)               # (its kernels need a GPU; the bookkeeping does not)
        g = torch.Generator().manual_seed(8)
        s.xyz_gradient_accum, s.denom, s.max_radii2D = torch.rand(P0, 1, generator=g), torch.rand(P0, 1, generator=g), torch.rand(P0, generator=g)
        stats.append(s)
    # ---- relayout_points: 9 new rows, 11 removed (one of them a new row), one gather
    mask = torch.zeros(P0 + 9, dtype=torch.bool)
    mask[torch.randperm(P0, generator=torch.Generator().manual_seed(1))[:10]] = True
    mask[P0 + 4] = True
    assert int(mask.sum()) == 11
    d = _new_rows(9, 21)
    maps = [tw[0].relayout_points(tw[2], remove_mask=mask, new_rows=_six(d), stats=s) for tw, s in zip((one, two), stats)]
    assert torch.equal(maps[0], maps[1]) and two[2].relayouts == 1
    P1 = P0 + 9 - 11
    _assert_equal(one, two, P1, "relayout_points")
    # appended rows start with zero moments, in both members
    new_at = torch.nonzero(maps[1] >= P0).reshape(-1)
    assert new_at.numel() == 8
    for name, (x, m, v) in _views(two[0], two[1], two[3]).items():
        if name != "other":
            assert not bool(m[new_at].any()) and not bool(v[new_at].any()) and bool(x[new_at].any()), name
    assert stats[1].denom.shape == (P1, 1) and not bool(stats[1].denom.any())
    # ---- a prune alone through the same call: the statistics ride along
    for s in stats:
        g = torch.Generator().manual_seed(9)
        s.xyz_gradient_accum, s.denom, s.max_radii2D = torch.rand(P1, 1, generator=g), torch.rand(P1, 1, generator=g), torch.rand(P1, generator=g)
    mask = torch.zeros(P1, dtype=torch.bool)
    mask[::6] = True
    for tw, s in zip((one, two), stats):
        tw[0].relayout_points(tw[2], remove_mask=mask, stats=s)
    P2 = P1 - int(mask.sum())
    _assert_equal(one, two, P2, "relayout_points, prune alone")
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(stats[0], k), getattr(stats[1], k)) and getattr(stats[1], k).shape[0] == P2 and bool(getattr(stats[1], k).any())
    # ---- densification_postfix, then prune_points
    d2 = _new_rows(6, 22)
    mask = torch.zeros(P2 + 6, dtype=torch.bool)
    mask[[0, 5, P2 + 1]] = True
    for tw, s in zip((one, two), stats):
        tw[0].densification_postfix(*_postfix_args(d2), tw[2], stats=s)
        tw[0].prune_points(mask, tw[2], stats=s)
    P3 = P2 + 6 - 3
    _assert_equal(one, two, P3, "densification_postfix + prune_points")
    # ---- reset_opacity: in place
    at = [o.flat_params.data_ptr() for o in two[3]]
    for tw in (one, two):
        tw[0].reset_opacity(tw[2])
    va, vb = _views(one[0], one[1], one[3]), _views(two[0], two[1], two[3])
    for name in va:
        for a, b in zip(va[name], vb[name]):
            assert torch.equal(a, b), name
    assert not bool(vb["opacity"][1].any()) and not bool(vb["opacity"][2].any()) and float(torch.sigmoid(vb["opacity"][0]).max()) <= 0.01 + 1e-7
    assert at == [o.flat_params.data_ptr() for o in two[3]]
    # ---- reorder_spatially
    perms = [tw[0].reorder_spatially(tw[2]) for tw in (one, two)]
    assert torch.equal(perms[0], perms[1]) and not torch.equal(perms[1], torch.arange(P3)) and two[0].spatially_ordered
    va, vb = _views(one[0], one[1], one[3]), _views(two[0], two[1], two[3])
    for name in va:
        for a, b in zip(va[name], vb[name]):
            assert torch.equal(a, b), name
    # ---- the densification event, both forms, on the group alone against the single optimizer
    from moss_amd.surgery import densification_event
    d3, d4 = _new_rows(4, 23), _new_rows(2, 24)
    mask = torch.zeros(P3 + 6, dtype=torch.bool)
    mask[[1, 2, P3 + 5]] = True
    r1 = densification_event(one[0], one[2], append=[_six(d3), _six(d4)], prune=mask, stats=stats[0], one_pass=False)
    r2 = densification_event(two[0], two[2], append=[_six(d3), _six(d4)], prune=mask, stats=stats[1], one_pass=True)
    assert r1["rows_after"] == r2["rows_after"] == P3 + 3 and two[2].relayouts == 3
    _assert_equal(one, two, P3 + 3, "densification_event", zeroed=("opacity",))     # (reset_opacity zeroed its moments)
    # what is not per-row kept values and moments; the Parameter objects, the schedule's rates and the SH degree survive
    for a, b in zip(other_before, _views(two[0], two[1], two[3])["other"]):
        assert torch.equal(a, b)
    assert objs == [[id(p) for p in o.bucket.params] for o in two[3]] and float(two[3][1].seg_lr[0]) == lr_xyz
    assert two[2].set_active_sh_degree(3) == 3 and two[2].rows == P3 + 3


def test_the_group_refuses_what_it_cannot_do(hip_lib):
    from moss_amd import dist as mdist
    from moss_amd.optim import FlatAdamW, FlatAdamWRows

    def opt(shapes, **kw):
        ps = [torch.nn.Parameter(torch.rand(s)) for s in shapes]
        return FlatAdamW([{"params": [p], "lr": 1e-3} for p in ps], mdist.GradBucket(ps, world=kw.get("shard", (0, 1))[1]), **kw), ps
    # members whose row-parameters have different row counts
    (a, pa), (b, pb) = opt([(8, 3), (8, 1)]), opt([(7, 3), (5,)])
    with pytest.raises(ValueError, match="different row counts"):
        FlatAdamWRows([a, b])
    # ... also when they drift apart later, by a call on a member behind the group's back
    (a, pa), (b, pb) = opt([(8, 3), (8, 1)]), opt([(8, 4), (5,)])
    rows = FlatAdamWRows([a, b])
    b.prune_rows(torch.arange(8) < 6)
    with pytest.raises(ValueError, match="different row counts"):
        rows.relayout_rows(torch.arange(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="different row counts"):
        rows.prune_rows(torch.ones(8, dtype=torch.bool))
    assert pa[0].shape[0] == 8                               # (refused before anything moved)
    # a sharded member: the single optimizer's message
    (a, pa), (s, ps) = opt([(8, 3)]), opt([(8, 3), (8, 1)], shard=(0, 2))
    with pytest.raises(RuntimeError, match="SHARDED FlatAdamW") as single:
        s.relayout_rows(torch.arange(8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="SHARDED FlatAdamW") as group:
        FlatAdamWRows([a, s])
    assert str(single.value) == str(group.value)
    # `appended` that does not name every row-parameter of every member
    (a, pa), (b, pb) = opt([(8, 3), (8, 1)]), opt([(8, 4), (5,)])
    rows = FlatAdamWRows([a, b])
    ident = torch.arange(10, dtype=torch.int32)
    with pytest.raises(ValueError, match="must name every parameter"):
        rows.relayout_rows(ident, {pa[0]: torch.zeros(2, 3), pa[1]: torch.zeros(2, 1)})              # (nothing of member 1)
    with pytest.raises(ValueError, match="must name every parameter"):
        rows.relayout_rows(ident, {pa[0]: torch.zeros(2, 3), pb[0]: torch.zeros(2, 4)})              # (one of member 0 is missing)
    with pytest.raises(ValueError, match="every row-parameter of every member"):
        rows.append_rows({pa[0]: torch.zeros(2, 3), pa[1]: torch.zeros(2, 1)})
    assert [int(p.shape[0]) for p in pa + pb] == [8, 8, 8, 5]
    rows.relayout_rows(ident, {pa[0]: torch.ones(2, 3), 1: torch.ones(2, 1), pb[0]: torch.ones(2, 4)})    # (by object or by index)
    assert [int(p.shape[0]) for p in pa + pb] == [10, 10, 10, 5] and rows.rows == 10
    # a parameter two members hold
    shared = torch.nn.Parameter(torch.rand(8, 3))
    m0 = FlatAdamW([{"params": [shared], "lr": 1e-3}], mdist.GradBucket([shared]))
    m1 = FlatAdamW([{"params": [shared], "lr": 1e-3}], mdist.GradBucket([shared]))
    with pytest.raises(ValueError, match="both hold one parameter"):
        FlatAdamWRows([m0, m1])


def test_more_than_twelve_descriptors_are_refused(hip_lib):
    """The limit is that of one ``moss_rows_relayout`` launch; a group holds to it on CPU tensors too, so that what passes here passes
    on the GPU."""
    from moss_amd import _lib
    from moss_amd import dist as mdist
    from moss_amd.optim import FlatAdamW, FlatAdamWRows
    members = []
    for k in range(2):
        ps = [torch.nn.Parameter(torch.rand(8, w + 1)) for w in range(5)]
        members.append(FlatAdamW([{"params": [p], "lr": 1e-3} for p in ps], mdist.GradBucket(ps)))
    rows = FlatAdamWRows(members)
    extra = [torch.rand(8, 1), torch.rand(8, 1), torch.rand(8)]
    assert len(rows.bucket.params) + len(extra) == _lib.ROWS_MAX_TENSORS + 1 == 13
    with pytest.raises(ValueError, match="more than 12 tensors in one launch"):
        rows.relayout_rows(torch.arange(6, dtype=torch.int32), extra=extra)
    assert all(int(p.shape[0]) == 8 for p in rows.bucket.params)
    out = rows.relayout_rows(torch.arange(6, dtype=torch.int32), extra=extra[:2])                  # (12 are carried)
    assert all(int(p.shape[0]) == 6 for p in rows.bucket.params) and torch.equal(out[1], extra[1][:6])


def test_event_with_context_and_graph_but_no_probe_is_refused_before_anything_is_touched(hip_lib):
    from moss_amd.surgery import densification_event
    pc, other, opt, members = _twin(True, hip_lib)

    class Stub:
        touched = 0

        def relearn_capacity(self):
            Stub.touched += 1

        def recapture(self, probe=None):
            Stub.touched += 1
    before = [o.flat_params.clone() for o in members]
    at = [o.flat_params.data_ptr() for o in members]
    prune = torch.zeros(P0, dtype=torch.bool)
    prune[3] = True
    for kw in (dict(prune=prune), dict(append=_six(_new_rows(2, 1))), dict(rows_changed=True)):
        with pytest.raises(ValueError, match="needs `probe`"):
            densification_event(pc, opt, context=Stub(), graphed=Stub(), probe=None, **kw)
    assert Stub.touched == 0 and at == [o.flat_params.data_ptr() for o in members]
    assert all(torch.equal(a, o.flat_params) for a, o in zip(before, members)) and pc._xyz.shape[0] == P0
    # what changes no shape needs no probe: the opacity reset is in place, and an empty mask moves nothing
    rep = densification_event(pc, opt, reset_opacity=True, prune=torch.zeros(P0, dtype=torch.bool), context=Stub(), graphed=Stub(), probe=None)
    assert not rep["recaptured"] and Stub.touched == 0 and at == [o.flat_params.data_ptr() for o in members]
