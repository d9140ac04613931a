"""``posefit.posed_frame`` is ``lbs.smpl_frame_fused`` followed by ``lbs.lbs_deform``, through the Python surface: the two share one
launcher per C entry point, so the outputs and the gradients that reach the frame's ``A_obs`` and ``d`` are the same bits.
(tests/test_gpu_pose_fit.py::test_existing_outputs_equal_the_old_entries shows the same of the C entry points themselves.)"""
import pytest
import torch

from moss_amd import lbs as mlbs
from moss_amd import posefit

pytestmark = pytest.mark.gpu

V, J = 300, 24


@pytest.mark.parametrize("P", [1, 129])                     # (129: one past the 128-Gaussian workgroup of the backward reductions)
@pytest.mark.parametrize("with_cR", [False, True])
@pytest.mark.parametrize("with_L", [False, True])
def test_posed_frame_is_smpl_frame_fused_then_lbs_deform(gpu, monkeypatch, P, with_cR, with_L):
    body = {k: v.to(gpu) for k, v in mlbs.synthetic_body_model(V, J, seed=40).items()}
    fr = {k: v.to(gpu) for k, v in mlbs.synthetic_frame(5, J).items()}
    big = {k: v.to(gpu) for k, v in mlbs.synthetic_frame(0, J, big_pose=True).items()}
    g = torch.Generator().manual_seed(P)
    ids = torch.randint(0, V, (P,), generator=g).to(gpu)
    x = (body["v_template"][ids] + 0.03 * torch.randn(P, 3, generator=g).to(gpu)).contiguous()
    L = (0.7 * torch.randn(P, J, generator=g)).to(gpu) if with_L else None
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g)).to(gpu).contiguous() if with_cR else None
    cot = [torch.randn(*s, generator=g).to(gpu) for s in ((P, 3, 3), (P, 3), (P, 3))]
    W, R, Th = body["weights"], fr["R"].reshape(3, 3).contiguous(), fr["Th"].reshape(3).contiguous()

    # the two ops, one after the other; A_obs and d as leaves so that their gradients can be read
    A_big, A_obs, d, _ = mlbs.smpl_frame_fused(body, fr, big, ids, correct_Rs=cR)
    A_obs, d = A_obs.detach().requires_grad_(True), d.detach().requires_grad_(True)
    two = mlbs.lbs_deform(ids, W, L, A_big, A_obs, d, R, Th, x=x)[:3]
    gA_two, gd_two = torch.autograd.grad(list(two), [A_obs, d], cot)

    # the one op; what its LBS backward hands its frame backward is recorded on the way
    seen = {}

    def spy(*args):
        seen.update(mlbs._launch_lbs_backward(*args))
        return seen

    monkeypatch.setattr(posefit, "_launch_lbs_backward", spy)
    leaves = {k: fr[k].clone().requires_grad_(True) for k in ("poses", "R", "Th")}
    one = posefit.posed_frame(body, W, {**fr, **leaves}, big, ids, x, lbs_offsets=L, correct_Rs=cR)
    torch.autograd.backward(list(one), cot)
    for name, a, b in zip(("T", "t", "p"), one, two):
        assert torch.equal(a, b), name
    assert torch.equal(seen["g_A_obs"], gA_two) and torch.equal(seen["g_d"], gd_two)
    assert all(bool(torch.isfinite(leaves[k].grad).all()) for k in leaves)
