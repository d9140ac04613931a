"""Saving, exporting and resuming ``moss_amd.train.MossStep`` (moss_amd/checkpoint.py) on the device: tests/test_gpu_moss_step.py's world
and helpers and tests/test_gpu_moss_step_events.py's scripted event (P = 6 890, 512 x 512, the 192 x 256 region).  A run that is stopped,
written to a file and continued in ANOTHER step must be the run that was never stopped, bit for bit -- eagerly and under a captured
graph, across a densification event, an SH-degree raise and a learning-rate change.  Every comparison is ``torch.equal`` or equality of
bytes."""
import copy
import os
from types import SimpleNamespace

import pytest
import torch

from tests.test_gpu_moss_step import FLAGS, _fresh, _gaussians, _load, _release_device_memory, _state, _step, world  # noqa: F401
from tests.test_gpu_moss_step_events import STATS, _assert_same, _scripted, low_degree_pc  # noqa: F401

pytestmark = pytest.mark.gpu


def _assert_identical(a, b, what):
    """Two steps: the five Gaussian tensors, the 68 network tensors, both moments of each, the three step counters, the three
    statistics, ``joint_F_sum``, ``lbs_weights_sum`` and ``terms`` (``_assert_same`` covers the flat buffers, counters, statistics, sums
    and terms; the tensors are compared through the Parameter objects as well, so a parameter that lost its home would show)."""
    from moss_amd.train import network_parameters
    _assert_same(a, b, what)
    for (n, p), q in zip(_gaussians(a.pc).items(), _gaussians(b.pc).values()):
        assert p.shape == q.shape and torch.equal(p, q), (what, n)
    na, nb = sum(network_parameters(a.pc), []), sum(network_parameters(b.pc), [])
    assert len(na) == len(nb) == 68
    for i, (p, q) in enumerate(zip(na, nb)):
        assert torch.equal(p, q), (what, "network tensor", i)
    for oa, ob in zip(a.optimizers, b.optimizers):
        for i in range(len(oa.bucket.params)):
            for x, y in zip(oa._moments_of(i), ob._moments_of(i)):
                assert torch.equal(x, y), (what, "moments", i)
        assert torch.equal(oa.step_state, ob.step_state) and oa.t == ob.t, what
        assert list(oa.seg_lr) == list(ob.seg_lr) and list(oa.seg_lr2) == list(ob.seg_lr2), what
        assert (oa.sh_active_degree, oa.sh_inactive_zero) == (ob.sh_active_degree, ob.sh_inactive_zero), what
    assert a.step_counts() == b.step_counts(), what
    assert a.pc.active_sh_degree == b.pc.active_sh_degree and a.pc.spatially_ordered == b.pc.spatially_ordered, what


def test_resume_eager(gpu, hip_lib, world, tmp_path):
    from moss_amd.checkpoint import load_checkpoint, save_checkpoint
    path = str(tmp_path / "run" / "chkpnt3.pth")
    pa, ca, sa = _fresh(world, stats=True)
    a = _step(world, pa, ca, sa)
    for k in range(3):
        _load(ca, k, gpu)
        a.compute()
    noise = torch.Generator().manual_seed(5).get_state()
    assert save_checkpoint(a, path, 3, extra={"generator": noise, "note": "after three"}) == path
    saved = [t.clone() for t in _state(a)]
    assert a.step_counts() == (3, 3, 3)
    for k in range(3):
        _load(ca, k, gpu)
        out_a = a.compute()
    # ---- a pristine copy in a new step
    pb, cb, sb = _fresh(world, stats=True)
    b = _step(world, pb, cb, sb)
    iteration, extra = load_checkpoint(b, path)
    assert iteration == 3 and extra["note"] == "after three" and torch.equal(extra["generator"], noise)
    assert b.step_counts() == (3, 3, 3) and b.graphed is None                       # no training step was taken by the load
    for j, (x, y) in enumerate(zip(saved, _state(b))):
        assert torch.equal(x, y), f"optimizer state {j} right after the load"
    for k in range(3):
        _load(cb, k, gpu)
        out_b = b.compute()
    torch.cuda.synchronize(gpu)
    _assert_identical(a, b, "three steps after the resume")
    assert torch.equal(out_a["render"], out_b["render"]) and float(out_b["render"].abs().max()) > 0.1
    assert a.step_counts() == (6, 6, 6) and float(sb.denom.max()) == 6.0 and bool(b.lbs_weights_sum.any())
    for s in (a, b):
        s.context.check_status()
        assert s.dropped_frames == 0
    # the file holds tensors and plain containers only
    payload = torch.load(path, weights_only=True)
    assert payload["format"] == "moss_amd.checkpoint" and payload["step"]["rows"] == 6890 and payload["step"]["version"] == 1

    def plain(x):
        if torch.is_tensor(x):
            return x.device.type == "cpu"
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, (list, tuple)):
            return all(plain(v) for v in x)
        return x is None or isinstance(x, (bool, int, float, str))
    assert plain(payload)


def test_resume_across_an_event_captured(gpu, hip_lib, world, low_degree_pc, tmp_path):
    from moss_amd.checkpoint import load_checkpoint, save_checkpoint
    path = str(tmp_path / "chkpnt.pth")
    low = dict(world, pc=low_degree_pc)
    pa, ca, sa = _fresh(low, stats=True)
    a = _step(world, pa, ca, sa).capture(warmup=2)
    P0 = int(pa._xyz.shape[0])

    def replay(step, k):
        _load(step.view, k, gpu)
        return step()
    replay(a, 0); replay(a, 1)
    report = a.densification_event(**_scripted(a.pc, 21))
    P1 = report["rows_after"]
    assert P1 != P0 and report["recaptured"]
    assert a.oneup_sh_degree() == 2
    a.set_learning_rates({"xyz": 1.1e-4, "features": (2e-3, 1.5e-4), "auto_regression": 2e-4})
    replay(a, 2); replay(a, 0)
    save_checkpoint(a, path, 4)
    saved = [t.clone() for t in _state(a)]
    assert a.step_counts() == (4, 4, 4)
    replay(a, 1)
    out_a = replay(a, 2)
    # ---- a pristine model at the original P, captured
    pb, cb, sb = _fresh(low, stats=True)
    b = _step(world, pb, cb, sb).capture(warmup=2)
    objects = list(_gaussians(pb).values()) + sum(b.network_params.values(), [])
    recaptures = b.recaptures
    assert int(pb._xyz.shape[0]) == P0 and b.step_counts() == (0, 0, 0) and pb.active_sh_degree == 1
    iteration, extra = load_checkpoint(b, path)
    assert iteration == 4 and extra is None
    assert b.step_counts() == (4, 4, 4)                                             # the saved counters: the load took no step
    assert b.recaptures == recaptures + 1
    assert [int(t.shape[0]) for t in _gaussians(pb).values()] == [P1] * 5 and b.rows.rows == P1
    for x, y in zip(objects, list(_gaussians(pb).values()) + sum(b.network_params.values(), [])):
        assert x is y                                                               # the Parameter objects B had
    for j, (x, y) in enumerate(zip(saved, _state(b))):
        assert x.shape == y.shape and torch.equal(x, y), f"optimizer state {j} right after the load"
    assert pb.active_sh_degree == 2 and b.opt_gaussians.sh_active_degree == 2 and b.opt_gaussians.fused.struct.sh_active_degree == 2
    assert b.context.fused_adamw is b.opt_gaussians.fused
    assert abs(b.opt_xyz.seg_lr[0] - 1.1e-4) < 1e-10 and abs(b.opt_networks.seg_lr[0] - 2e-4) < 1e-10
    assert sb.denom.shape == (P1, 1) and float(sb.denom.max()) == 2.0 and b.lbs_weights_sum.shape[-2] == P1
    replay(b, 1)
    out_b = replay(b, 2)
    torch.cuda.synchronize(gpu)
    _assert_identical(a, b, "two replays after the resume")
    assert torch.equal(out_a["render"], out_b["render"]) and float(out_b["render"].abs().max()) > 0.1
    assert a.step_counts() == (6, 6, 6)
    f = pb._features.detach()
    assert bool(f[:, 4:9].any()) and not bool(f[:, 9:].any())                       # degree 2 trains, degree 3 is exactly zero still
    for s in (a, b):
        s.check()
        assert s.dropped_frames == 0


def test_export_to_the_model_directory(gpu, hip_lib, world, tmp_path):
    from moss_amd.checkpoint import load_scene, save_scene
    from moss_amd.diff_gaussian_rasterization import RasterContext
    from moss_amd.gaussian_renderer import render
    from tests.test_checkpoint_cpu import _expected_bytes
    root = str(tmp_path / "model")
    pc, cam, _ = _fresh(world)
    step = _step(world, pc, cam)
    for k in range(2):
        _load(cam, k, gpu)
        step.compute()
    _load(cam, 2, gpu)
    ply, ckpt = save_scene(root, 2, pc)
    with torch.no_grad():
        image = render(cam, pc, step.pipe, world["bg"])["render"].clone()
    assert open(ply, "rb").read() == _expected_bytes(pc, 3)                         # the layout computed here from the device tensors
    assert os.path.getsize(ply) == len(_expected_bytes(pc, 3)) and ckpt.endswith(os.path.join("mlp_ckpt", "iteration_2", "ckpt.pth"))
    # ---- into a fresh model
    pc2, cam2, _ = _fresh(world)
    assert not torch.equal(pc2._xyz, pc._xyz)
    assert load_scene(root, pc2) == 2
    for (n, p), q in zip(_gaussians(pc).items(), _gaussians(pc2).values()):
        assert torch.equal(p, q) and q.is_cuda, n
    for m in ("auto_regression", "cross_attention_lbs"):
        for (n, p), (_, q) in zip(getattr(pc, m).state_dict().items(), getattr(pc2, m).state_dict().items()):
            assert torch.equal(p, q), (m, n)
    _load(cam2, 2, gpu)
    cx = RasterContext()
    cx.set_async(True)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, raster_context=cx, **FLAGS)
    with torch.no_grad():
        image2 = render(cam2, pc2, pipe, world["bg"])["render"]
    torch.cuda.synchronize(gpu)
    assert torch.equal(image, image2) and float(image.abs().max()) > 0.1
    step.context.check_status()


def test_refusals_leave_the_step_untouched(gpu, hip_lib, world):
    pa, ca, sa = _fresh(world, stats=True)
    a = _step(world, pa, ca, sa)
    a.compute()
    sd = a.state_dict()
    pb, cb, sb = _fresh(world, stats=True)
    b = _step(world, pb, cb, sb)
    _load(cb, 1, gpu)
    b.compute()
    pc_, cc, _ = _fresh(world)
    c = _step(world, pc_, cc)                                                         # built without stats
    c.compute()
    torch.cuda.synchronize(gpu)

    def everything(s):
        out = [t.clone() for t in _state(s)] + [s._terms.clone(), s.joint_F_sum.clone()]
        # (the sum of the LBS weights is kept with the statistics: a step built without them has none)
        return out + ([s.lbs_weights_sum.clone()] + [getattr(s.stats, k).clone() for k in STATS] if s.stats is not None else [])

    def changed(key, edit):
        bad = dict(sd)
        bad[key] = copy.deepcopy(sd[key])
        bad[key] = edit(bad[key])
        return bad

    def swap(groups):
        return [groups[1], groups[0]] + groups[2:]

    def widen(groups):
        return [[groups[0][0], [groups[0][1][0] + 1, 3]]] + groups[1:]

    def rename(nets):
        nets["auto_regression"][5][0] = "block_mlps.9.bias"
        return nets

    def reshape(nets):
        nets["cross_attention_lbs"][0][1] = nets["cross_attention_lbs"][0][1][::-1]
        return nets
    cases = [("version", changed("version", lambda v: v + 1), b), ("max_sh_degree", changed("max_sh_degree", lambda d: 2), b),
             ("gaussians", changed("gaussians", swap), b), ("gaussians", changed("gaussians", widen), b),
             ("networks", changed("networks", rename), b), ("networks", changed("networks", reshape), b),
             ("stats", changed("stats", lambda s: None), b), ("stats", sd, c), ("unified_features", changed("unified_features", lambda u: False), b)]
    for field, bad, target in cases:
        before, counts = everything(target), target.step_counts()
        with pytest.raises(ValueError, match=field):
            target.load_state_dict(bad)
        torch.cuda.synchronize(gpu)
        for j, (x, y) in enumerate(zip(before, everything(target))):
            assert torch.equal(x, y), (field, j)
        assert target.step_counts() == counts == (1, 1, 1) and target.graphed is None
    # ... and the state itself is good: b takes it and is a
    b.load_state_dict(sd)
    torch.cuda.synchronize(gpu)
    _assert_identical(a, b, "after the load that is not refused")
