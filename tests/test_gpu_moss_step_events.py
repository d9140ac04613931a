"""Densification events and SH-degree raises ON ``moss_amd.train.MossStep`` -- the step whose Gaussians sit in two optimizers -- and
MOSS's schedule around it (``train.run_schedule``).  tests/test_gpu_moss_step.py's scene, frames and fixtures (P = 6 890, 512 x 512, the
192 x 256 region).  Every comparison is bit for bit: the events add no arithmetic, so any difference is a bug.  Every test ends with
``dropped_frames == 0``: the probe sizes the binning capacity on the very frame that is replayed."""
import copy
import math

import pytest
import torch

from tests.test_gpu_moss_step import _fresh, _load, _release_device_memory, _state, _step, world  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

STATS = ("xyz_gradient_accum", "denom", "max_radii2D")


def _scripted(pc, seed, n_clone=300, n_split=100, n_prune=300):
    """A deterministic decision from the CURRENT parameters and a seeded generator: ``n_clone`` clones, ``n_split`` Gaussians split in
    two (their sources pruned, ``scene/gaussian_model.py:526-527``) and ``n_prune`` more rows pruned, over the set after the appends."""
    g = torch.Generator().manual_seed(seed)
    dev = pc._xyz.device
    P = int(pc._xyz.shape[0])

    def rows(t, idx, times=1):
        x = t.detach()[idx]
        return x.repeat(times, *([1] * (x.dim() - 1))).clone()
    src = torch.randperm(P, generator=g)[:n_clone].to(dev)
    clone = {"new_xyz": rows(pc._xyz, src), "new_features_dc": rows(pc._features_dc, src), "new_features_rest": rows(pc._features_rest, src),
             "new_opacities": rows(pc._opacity, src), "new_scaling": rows(pc._scaling, src), "new_rotation": rows(pc._rotation, src)}
    src2 = torch.randperm(P, generator=g)[:n_split].to(dev)
    noise = (0.01 * torch.randn(2 * n_split, 3, generator=g)).to(dev)
    split = {"new_xyz": rows(pc._xyz, src2, 2) + noise, "new_features_dc": rows(pc._features_dc, src2, 2),
             "new_features_rest": rows(pc._features_rest, src2, 2), "new_opacities": rows(pc._opacity, src2, 2),
             "new_scaling": rows(pc._scaling, src2, 2) - math.log(1.6), "new_rotation": rows(pc._rotation, src2, 2)}
    total = P + n_clone + 2 * n_split
    prune = torch.zeros(total, dtype=torch.bool)
    prune[src2.cpu()] = True
    prune[torch.randperm(total, generator=g)[:n_prune]] = True
    return {"append": [clone, split], "prune": prune.to(dev)}


def _statistics(step):
    return [getattr(step.stats, k) for k in STATS] + [step.joint_F_sum, step.lbs_weights_sum]


def _assert_same(a, b, what=""):
    """Two steps: the three optimizers' flat buffers and step counters, the statistics and sums, the loss terms."""
    for j, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: optimizer state {j} (parameters, exp_avg, exp_avg_sq, counter per optimizer)"
    for j, (x, y) in enumerate(zip(_statistics(a), _statistics(b))):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: statistic {j}"
    assert torch.equal(a.terms, b.terms), what


def _pair(world, gpu, steps, pristine=None):
    """Two steps on deep copies of one model, taken through the same ``steps`` eager iterations."""
    out = []
    for _ in range(2):
        pc, cam, st = _fresh(world if pristine is None else dict(world, pc=pristine), stats=True)
        step = _step(world, pc, cam, st)
        for _ in range(steps):
            step.compute()
        out.append(step)
    torch.cuda.synchronize(gpu)
    _assert_same(*out, "before the event")
    return out


@pytest.fixture(scope="module")
def low_degree_pc(gpu, world):
    """The model at SH degree 1 with ``zero_inactive_sh=True``: MOSS's state below the maximum degree."""
    from moss_amd import scenes
    w = world["pc"]
    pc = type(w)(scenes.config2(), sh_degree=1, device=gpu, unified_features=True, zero_inactive_sh=True)
    pc.SMPL_NEUTRAL, pc.knn, pc.motion_offset_flag = w.SMPL_NEUTRAL, w.knn, True
    pc.auto_regression, pc.cross_attention_lbs = copy.deepcopy(w.auto_regression), copy.deepcopy(w.cross_attention_lbs)
    assert pc.active_sh_degree == 1 and not bool(pc._features[:, 4:].any()) and bool(pc._features[:, :4].any())
    return pc


def test_one_gather_launch_equals_the_per_optimizer_primitives(gpu, hip_lib, world):
    """The scripted event -- 300 clones, 200 split rows, ~400 pruned -- with ``one_pass=True`` (ONE ``moss_rows_relayout`` launch over
    both optimizers) against ``one_pass=False`` (``append_rows`` / ``prune_rows`` per optimizer)."""
    a, b = _pair(world, gpu, 3)
    P = int(a.pc._xyz.shape[0])
    event = _scripted(a.pc, 11)
    assert 380 <= int(event["prune"].sum()) <= 400
    ra = a.densification_event(one_pass=True, **event)
    rb = b.densification_event(one_pass=False, **event)
    torch.cuda.synchronize(gpu)
    assert ra["relayouts"] == 1 and rb["relayouts"] == 0
    assert ra["rows_before"] == rb["rows_before"] == P and ra["rows_after"] == rb["rows_after"] == P + 500 - int(event["prune"].sum())
    assert not ra["recaptured"] and not rb["recaptured"]
    _assert_same(a, b, "after the event")
    P1 = ra["rows_after"]
    for s in (a, b):
        pc = s.pc
        assert [int(t.shape[0]) for t in (pc._xyz, pc._features, pc._opacity, pc._scaling, pc._rotation)] == [P1] * 5
        assert s.step_counts() == (3, 3, 3)
        assert s.stats.denom.shape == (P1, 1) and not bool(s.stats.denom.any())
        assert s.lbs_weights_sum.shape[-2] == P1 and not bool(s.lbs_weights_sum.any()) and not bool(s.joint_F_sum.any())
        assert s.opt_gaussians.fused is not None and s.context.fused_adamw is s.opt_gaussians.fused
    # the appended rows' moments are zero, the surviving rows' are not
    m, v = a.opt_xyz._moments_of(0)
    kept = int((~event["prune"][:P]).sum())
    assert bool(m[:kept].any()) and bool(v[:kept].any()) and not bool(m[kept:].any()) and not bool(v[kept:].any())
    # ... and both go on, alike
    for s in (a, b):
        s.compute()
    torch.cuda.synchronize(gpu)
    _assert_same(a, b, "one step later")
    for s in (a, b):
        s.context.check_status()
        assert s.dropped_frames == 0 and s.step_counts() == (4, 4, 4)


def test_the_captured_step_goes_on_after_an_event(gpu, hip_lib, world):
    g, e = _pair(world, gpu, 3)
    g.capture(warmup=2)
    event = _scripted(g.pc, 12)
    report = g.densification_event(**event)
    e.densification_event(**event)
    assert report["recaptured"] and g.graphed.recaptures == 1 and report["relayouts"] == 1
    assert report["event_ms"] >= report["probe_ms"] + report["capture_ms"] > 0
    assert g.graphed.captured_capacity == g.context.capacity > 0
    _assert_same(g, e, "after the event")                                # (the re-capture took no training step)
    for i in range(3):                                                   # (the frame the probe sized the capacity on)
        out_g = g()
        out_e = e.compute()
        torch.cuda.synchronize(gpu)
        assert torch.equal(out_g["render"], out_e["render"]) and float(out_g["render"].abs().max()) > 0.1, i
        _assert_same(g, e, f"replay {i} after the event")
    assert g.check() is False and g.dropped_frames == 0
    e.context.check_status()
    assert g.step_counts() == e.step_counts() == (6, 6, 6) and float(g.stats.denom.max()) == 3.0


def test_moss_decision_through_the_step_equals_the_single_optimizer_path(gpu, hip_lib, world):
    """``step.densify_and_prune`` against ``densify_and_prune_fused`` on one unfused ``FlatAdamW`` that holds copies of all five tensors,
    their moments and the statistics.  The thresholds come from the state itself so that the phases have something to select: the
    gradient threshold is the median accumulated gradient, the clone / split boundary the median scale, the opacity threshold the
    30 % quantile of the opacities."""
    from moss_amd import dist as mdist
    from moss_amd.densify import DensifyStats, densify_and_prune_fused
    from moss_amd.optim import FlatAdamW
    a = _pair(world, gpu, 3)[0]
    pc = a.pc
    names = ("_xyz", "_features", "_opacity", "_scaling", "_rotation")
    # ---- the single-optimizer copy
    pc2 = copy.deepcopy(world["pc"])
    bucket2 = mdist.GradBucket([getattr(pc2, n) for n in names])
    opt2 = FlatAdamW(pc2.param_groups(), bucket2, eps=1e-15, weight_decay=0.01, capturable=True)

    def moments(step_or_opt, p):
        for o in ([step_or_opt] if isinstance(step_or_opt, FlatAdamW) else [a.opt_gaussians, a.opt_xyz]):
            idx = {id(q): i for i, q in enumerate(o.bucket.params)}
            if id(p) in idx:
                return o._moments_of(idx[id(p)])
        raise KeyError
    with torch.no_grad():
        for n in names:
            getattr(pc2, n).copy_(getattr(pc, n))
            for dst, src in zip(moments(opt2, getattr(pc2, n)), moments(a, getattr(pc, n))):
                dst.copy_(src)
    P = int(pc._xyz.shape[0])
    stats2 = DensifyStats(P, gpu)
    for k in STATS:
        getattr(stats2, k).copy_(getattr(a.stats, k))
    joint_F, lbs_w = a.joint_F_sum.clone(), a.lbs_weights_sum.clone()
    assert bool(joint_F.any()) and bool(lbs_w.any()) and float(stats2.denom.max()) == 3.0
    # ---- thresholds from the state
    grads = a.stats.mean_grads().reshape(-1)
    args = dict(max_grad=float(grads.median()), min_opacity=float(torch.sigmoid(pc._opacity.detach()).quantile(0.3)),
                extent=100.0 * float(torch.exp(pc._scaling.detach()).max(dim=1).values.median()), max_screen_size=None)
    gens = [torch.Generator(device=gpu).manual_seed(5) for _ in range(2)]
    r2 = densify_and_prune_fused(pc2, opt2, stats2, joint_F, lbs_w, args["max_grad"], args["min_opacity"], args["extent"], None,
                                 a.view.big_pose_world_vertex, generator=gens[0], one_pass=True)
    r1 = a.densify_and_prune(generator=gens[1], **args)
    torch.cuda.synchronize(gpu)
    print("\ndecision " + ", ".join(f"{k} {r1[k]}" for k in ("rows_before", "cloned", "split", "merged", "pruned", "rows_after", "relayouts", "host_reads")))
    for k in ("rows_before", "cloned", "split", "merged", "pruned", "rows_after", "relayouts"):
        assert r1[k] == r2[k], k
    assert r1["cloned"] > 0 or r1["split"] > 0 or r1["pruned"] > 0       # (the test cannot pass by doing nothing)
    assert r1["rows_after"] != P and 1 <= r1["relayouts"] <= 4 and not r1["recaptured"]
    P1 = r1["rows_after"]
    for n in names:
        p1, p2 = getattr(pc, n), getattr(pc2, n)
        assert p1.shape == p2.shape and p1.shape[0] == P1 and torch.equal(p1, p2), n
        for x, y, part in zip(moments(a, p1), moments(opt2, p2), ("exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), (n, part)
    for k in STATS:
        assert getattr(a.stats, k).shape[0] == P1 and torch.equal(getattr(a.stats, k), getattr(stats2, k)), k
    assert not bool(a.joint_F_sum.any()) and a.lbs_weights_sum.shape == lbs_w.shape[:-2] + (P1, lbs_w.shape[-1]) and not bool(a.lbs_weights_sum.any())
    assert a.step_counts() == (3, 3, 3) and opt2.step_count() == 0
    # the step goes on at the new size
    out = a.compute()
    torch.cuda.synchronize(gpu)
    a.context.check_status()
    assert a.dropped_frames == 0 and bool(torch.isfinite(out["terms"]).all()) and float(a.stats.denom.max()) == 1.0
    # built without statistics there is nothing to decide on
    pc3, cam3, _ = _fresh(world)
    with pytest.raises(RuntimeError, match="without stats"):
        _step(world, pc3, cam3).densify_and_prune(**args)


def test_reset_opacity_alone_keeps_the_captured_graph(gpu, hip_lib, world):
    g, e = _pair(world, gpu, 3)
    g.capture(warmup=2)
    graph, outputs = g.graphed.graph, g.graphed.outputs
    at = [o.flat_params.data_ptr() for o in g.optimizers]
    old = g.pc._opacity.detach().clone()
    report = g.densification_event(reset_opacity=True)
    e.densification_event(reset_opacity=True)
    assert not report["recaptured"] and g.graphed.graph is graph and g.graphed.outputs is outputs and g.graphed.recaptures == 0
    assert at == [o.flat_params.data_ptr() for o in g.optimizers] and report["relayouts"] == 0
    m, v = g.opt_gaussians._moments_of([id(p) for p in g.opt_gaussians.bucket.params].index(id(g.pc._opacity)))
    assert not bool(m.any()) and not bool(v.any())
    low = torch.min(torch.sigmoid(old), torch.ones_like(old) * 0.01)     # scene/gaussian_model.py:314-317
    assert torch.equal(g.pc._opacity.detach(), torch.log(low / (1 - low))) and float(torch.sigmoid(g.pc._opacity.detach()).max()) <= 0.01 + 1e-7
    assert bool(g.opt_gaussians.exp_avg.any()) and bool(g.joint_F_sum.any())     # (nothing else was reset)
    _assert_same(g, e, "after the reset")
    g()
    e.compute()
    torch.cuda.synchronize(gpu)
    _assert_same(g, e, "the replay after the reset")
    assert bool(m.any()) and g.check() is False and g.dropped_frames == 0 and g.step_counts() == (4, 4, 4)


def test_oneup_sh_degree_reaches_the_model_the_optimizer_and_the_capture(gpu, hip_lib, world, low_degree_pc):
    g, e = _pair(world, gpu, 2, pristine=low_degree_pc)
    assert g.opt_gaussians.sh_active_degree == 1 and g.opt_gaussians.sh_inactive_zero
    g.capture(warmup=2)
    assert g.oneup_sh_degree() == 2 and e.oneup_sh_degree() == 2
    assert g.pc.active_sh_degree == 2 and g.opt_gaussians.sh_active_degree == 2 and g.opt_gaussians.fused.struct.sh_active_degree == 2
    assert g.graphed.recaptures == 1 and e.graphed is None
    assert not bool(g.pc._features[:, 4:].any())
    for i in range(2):
        g()
        e.compute()
        torch.cuda.synchronize(gpu)
        _assert_same(g, e, f"replay {i} at degree 2")
    f = g.pc._features.detach()
    assert bool(f[:, 4:9].any())                                         # the new coefficients train: not frozen behind a stale degree
    assert int((f[:, 4:9].abs().sum(dim=(1, 2)) > 0).sum()) > 100
    i_sh = [id(p) for p in g.opt_gaussians.bucket.params].index(id(g.pc._features))
    m, v = g.opt_gaussians._moments_of(i_sh)
    assert bool(m[:, 4:9].any()) and bool(v[:, 4:9].any())
    assert not bool(f[:, 9:].any()) and not bool(m[:, 9:].any()) and not bool(v[:, 9:].any())      # degree 3: exactly zero still
    assert g.check() is False and g.dropped_frames == 0 and g.step_counts() == (4, 4, 4)
    # capped at 3, and nothing is captured again for a raise that is none
    assert g.oneup_sh_degree() == 3 and g.graphed.recaptures == 2
    assert g.oneup_sh_degree() == 3 and g.graphed.recaptures == 2


def test_run_schedule_in_miniature_equals_the_loop_written_out(gpu, hip_lib, world, low_degree_pc):
    """12 iterations of MOSS's loop order, events at 4 and 8 (``interval=4``, ``densify_from=3``, ``densify_until=11``), degree raises at
    5 and 10, three frames drawn without replacement: the captured step under ``run_schedule`` against a plain loop of ``compute()``."""
    from moss_amd.train import frame_order, run_schedule
    g, e = _pair(world, gpu, 1, pristine=low_degree_pc)
    g.capture(warmup=2)

    def decision(step, i):
        return step.densification_event(**_scripted(step.pc, 100 + i, n_clone=120, n_split=40, n_prune=90))
    seen = []
    report = run_schedule(g, 3, 12, densify_from=3, densify_until=11, interval=4, sh_every=5, on_event=lambda s, i: decision(s, i),
                          load_frame=lambda k: (seen.append(k), _load(g.view, k, gpu)))
    # ---- the same, written out
    order = frame_order(3, 12)
    assert seen == order and sorted(order[:3]) == sorted(order[3:6]) == [0, 1, 2]        # without replacement
    sizes = []
    for i in range(1, 13):
        if i % 5 == 0:
            e.oneup_sh_degree()
        _load(e.view, order[i - 1], gpu)
        e.compute()
        if 3 < i < 11 and i % 4 == 0:
            sizes.append(decision(e, i)["rows_after"])
    torch.cuda.synchronize(gpu)
    _assert_same(g, e, "after 12 iterations")
    assert [ev["iteration"] for ev in report["events"]] == [4, 8] and [ev["rows_after"] for ev in report["events"]] == sizes
    assert all(ev["recaptured"] and ev["relayouts"] == 1 for ev in report["events"])
    assert report["sh_raises"] == 2 and g.pc.active_sh_degree == e.pc.active_sh_degree == 3
    # (two events, two raises; a check() on the way may add one: the three frames do not need the same room)
    assert report["recaptures"] == g.graphed.recaptures >= 4 and report["opacity_resets"] == 0
    assert report["rows"] == sizes[-1] == int(g.pc._xyz.shape[0]) and report["iterations"] == 12
    assert [report["phases"][k]["iterations"] for k in ("before", "during", "after")] == [3, 7, 2] and report["seconds"] > 0
    g.check()
    assert report["dropped_frames"] == g.dropped_frames == 0
    e.context.check_status()
    assert g.step_counts() == e.step_counts() == (13, 13, 13)
