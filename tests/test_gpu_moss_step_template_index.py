"""``MossStep(template_index=True)``: the nearest-vertex query of the LBS deformation through a ``knn_cuda.TemplateIndex`` built once,
against the same step without it -- eagerly, captured, across frames and across a densification event that changes P.  The index
returns the ids the cell grid returns, so everything is compared bit for bit.  The scene, frames and fixtures of
tests/test_gpu_moss_step.py (P = 6 890, 512 x 512, the 192 x 256 region); the event of tests/test_gpu_moss_step_events.py."""
import pytest
import torch

from tests.test_gpu_moss_step import LRS, _fresh, _load, _release_device_memory, _state, world  # noqa: F401  (fixtures and helpers)
from tests.test_gpu_moss_step_events import _scripted, _statistics

pytestmark = pytest.mark.gpu


def _same(a, b, out_a, out_b, what):
    for j, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: optimizer state {j} (parameters, exp_avg, exp_avg_sq, counter per optimizer)"
    for j, (x, y) in enumerate(zip(_statistics(a), _statistics(b))):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: statistic {j}"
    assert torch.equal(a.terms, b.terms), what
    assert torch.equal(out_a["render"], out_b["render"]) and float(out_a["render"].abs().max()) > 0.1, what


def test_the_step_with_a_template_index_is_the_step_without(gpu, hip_lib, world):
    from moss_amd.knn_cuda import TemplateIndex
    from moss_amd.train import MossStep
    steps = []
    for flag in (False, True):
        pc, cam, st = _fresh(world, stats=True)
        steps.append(MossStep(pc, cam, world["gt"], world["bkgd"], world["region"], world["bg"], world["lpips"], LRS, stats=st,
                              template_index=flag))
    plain, indexed = steps
    assert plain.template_index is None and getattr(plain.pc, "template_index", None) is None
    assert isinstance(indexed.template_index, TemplateIndex) and indexed.pc.template_index is indexed.template_index
    assert indexed.template_index.V == int(indexed.view.big_pose_world_vertex.shape[-2])
    for i in range(3):
        outs = [s.compute() for s in steps]
        torch.cuda.synchronize(gpu)
        _same(plain, indexed, *outs, f"eager step {i}")
    for s in steps:
        s.capture(warmup=2)
    for i in range(4):
        for s in steps:
            _load(s.view, i % 3, gpu)
        outs = [s() for s in steps]
        torch.cuda.synchronize(gpu)
        _same(plain, indexed, *outs, f"replay {i}")
    P = int(plain.pc._xyz.shape[0])
    event = _scripted(plain.pc, 21)
    reports = [s.densification_event(**event) for s in steps]
    assert all(r["recaptured"] for r in reports) and reports[0]["rows_after"] == reports[1]["rows_after"] != P
    assert indexed.pc.template_index is indexed.template_index              # (it does not depend on P: the event keeps it)
    for i in range(2):
        outs = [s() for s in steps]
        torch.cuda.synchronize(gpu)
        _same(plain, indexed, *outs, f"replay {i} after the event")
    assert plain.check() == indexed.check()
    assert plain.dropped_frames == indexed.dropped_frames
    assert plain.step_counts() == indexed.step_counts() == (9, 9, 9)
