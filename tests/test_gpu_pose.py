"""The fused pose-refinement head and matrix-Fisher NLL on the device (C ABI moss_pose_head_forward / _backward,
moss_matrix_fisher_nll; moss_amd.pose): the kernels against the reference's own float64 numbers (tests/golden/pose_head.npz),
determinism, every gradient written, capture in a hipGraph with a new frame per replay, and the renderer's ``pipe.pose_head_in_op``.

The bars.  Beside every float64 result X the fixture stores X_err32: what the REFERENCE loses when it runs in float32 on the same
inputs.  A kernel result may be off by K = 8 times that (the project's parity factor: a float32 computation with another summation
order, no better and no worse than the reference's own).  Nothing here is tuned to the kernels.  U and V are never compared: Rs is
within 1e-5 of a rotation, so they are not unique.  Each test prints the worst ratio of error to err32 it met.
"""
import ctypes

import numpy as np
import pytest
import torch

from moss_amd import lbs as mlbs
from moss_amd import pose as mpose
from tests.test_pose_cpu import GENERAL_CASES, GOLDEN, HEAD_CASES, head_case, head_loss

pytestmark = pytest.mark.gpu

K = 8.0


def _net(params, dev):
    net = mpose.head_module()
    net.load_state_dict({k: v.float() for k, v in params.items()})
    return net.to(dev)


def _err(got, ref):
    return float(np.abs(got.detach().double().cpu().numpy() - np.asarray(ref, dtype=np.float64)).max())


@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_matches_reference_float64(gpu, hip_lib, case):
    """pose_head_fused: Rs, the proper singular values, nll and the gradient of 0.06 nll.mean() + <Rs, g_Rs> w.r.t. each of the 52
    parameters, against the reference's float64 run, each within K x the reference's own float32 error of that quantity."""
    g = np.load(GOLDEN)
    params, poses, target_R, g_Rs = head_case(g, case, dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    out = mpose.pose_head_fused(net, poses, target_R)
    assert set(out) == {"Rs", "pose_S", "nll", "target_R"}
    assert out["Rs"].shape == (23, 3, 3) and out["pose_S"].shape == (23, 3) and out["nll"].shape == (23,)
    assert not out["pose_S"].requires_grad
    head_loss(out["Rs"], out["nll"], g_Rs).backward()
    ratios = {"Rs": _err(out["Rs"], g[f"{case}_Rs"]) / float(g[f"{case}_Rs_err32"]),
              "S": _err(out["pose_S"], g[f"{case}_S"]) / float(g[f"{case}_S_err32"]),
              "nll": _err(out["nll"], g[f"{case}_nll"]) / float(g[f"{case}_nll_err32"])}
    grad_err32 = g[f"{case}_grad_err32"]
    worst_grad, worst_name = 0.0, None
    for i, (name, p) in enumerate(zip(mpose.PARAM_NAMES, mpose.head_parameters(net))):
        assert p.grad is not None and p.grad.shape == p.shape, name
        r = _err(p.grad, g[f"{case}_grad_{name}"]) / float(grad_err32[i])
        if r > worst_grad:
            worst_grad, worst_name = r, name
    ratios["grad"] = worst_grad
    print(f"\n{case}: error / err32: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" (worst gradient: {worst_name})")
    assert max(ratios.values()) < K, ratios


@pytest.mark.parametrize("case", GENERAL_CASES)
def test_general_nll_matches_reference_float64(gpu, hip_lib, case):
    """matrix_fisher_nll_fused on general matrices (both determinant signs, singular values up to ~80): nll and d nll.mean() / dF."""
    g = np.load(GOLDEN)
    F = torch.from_numpy(g[f"{case}_F"]).to(gpu).requires_grad_(True)
    target_R = torch.from_numpy(g[f"{case}_target_R"]).to(gpu)
    nll = mpose.matrix_fisher_nll_fused(F, target_R)
    assert nll.shape == (23,)
    nll.mean().backward()
    ratios = {"nll": _err(nll, g[f"{case}_nll"]) / float(g[f"{case}_nll_err32"]),
              "dF": _err(F.grad, g[f"{case}_dF"]) / float(g[f"{case}_dF_err32"])}
    print(f"\n{case}: error / err32: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) < K, ratios
    # without a gradient the same values come from the forward-only launch
    assert torch.equal(mpose.matrix_fisher_nll_fused(F.detach(), target_R), nll.detach())


def _run_head(net, poses, target_R, g_Rs):
    out = mpose.pose_head_fused(net, poses, target_R)
    grads = torch.autograd.grad(head_loss(out["Rs"], out["nll"], g_Rs), mpose.head_parameters(net))
    return [out["Rs"].detach(), out["pose_S"].detach(), out["nll"].detach()] + [x.detach() for x in grads]


def test_deterministic(gpu, hip_lib):
    """Two calls on the same inputs: bit-identical Rs, S, nll and all 52 gradients; the same for the standalone NLL."""
    g = np.load(GOLDEN)
    params, poses, target_R, g_Rs = head_case(g, "trained_large", dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    a = [v.clone() for v in _run_head(net, poses, target_R, g_Rs)]
    b = _run_head(net, poses, target_R, g_Rs)
    assert len(a) == 55
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
    res = []
    for _ in range(2):
        F = torch.from_numpy(g["g5_F"]).to(gpu).requires_grad_(True)
        nll = mpose.matrix_fisher_nll_fused(F, torch.from_numpy(g["g5_target_R"]).to(gpu))
        nll.sum().backward()
        res.append((nll.detach().clone(), F.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_every_gradient_is_written(gpu, hip_lib):
    """Through the C ABI: the 52 gradient buffers are pre-filled with NaN; the backward leaves none (it writes, never accumulates) --
    also with g_Rs and g_nll NULL, when every gradient is zero."""
    from moss_amd._lib import POSE_HEAD_SAVED_FLOATS, PoseHeadArgs, PoseHeadBackwardArgs, check
    g = np.load(GOLDEN)
    params, poses, target_R, g_Rs = head_case(g, "trained_small", dtype=torch.float32, device=gpu)
    plist = [params[k].contiguous() for k in mpose.PARAM_NAMES]
    poses = poses.reshape(72).contiguous()
    Rs, S, nll = torch.empty(23, 3, 3, device=gpu), torch.empty(23, 3, device=gpu), torch.empty(23, device=gpu)
    saved = torch.empty(POSE_HEAD_SAVED_FLOATS, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    a = PoseHeadArgs()
    mpose._fill_head(a, poses, target_R, 1.005, mlbs.SMPL_PARENTS, plist)
    a.Rs, a.S, a.nll, a.saved = Rs.data_ptr(), S.data_ptr(), nll.data_ptr(), saved.data_ptr()
    check(hip_lib.moss_pose_head_forward(ctypes.byref(a), stream), "forward")
    g_nll = torch.full((23,), 0.06 / 23, device=gpu)
    for with_cotangents in (True, False):
        grads = [torch.full_like(p, float("nan")) for p in plist]
        b = PoseHeadBackwardArgs()
        mpose._fill_head(b, poses, target_R, 1.005, mlbs.SMPL_PARENTS, plist)
        b.S, b.saved = S.data_ptr(), saved.data_ptr()
        if with_cotangents:
            b.g_Rs, b.g_nll = g_Rs.data_ptr(), g_nll.data_ptr()
        for i, t in enumerate(grads):
            b.grads[i] = t.data_ptr()
        check(hip_lib.moss_pose_head_backward(ctypes.byref(b), stream), "backward")
        torch.cuda.synchronize(gpu)
        for name, t in zip(mpose.PARAM_NAMES, grads):
            assert not bool(torch.isnan(t).any()), name
            if not with_cotangents:
                assert not bool(t.any()), name
    # the argument checks of the C ABI
    b.grads[51] = None
    assert hip_lib.moss_pose_head_backward(ctypes.byref(b), stream) == -1 and b"52" in hip_lib.moss_last_error()
    a.fc_in[22] = 3
    assert hip_lib.moss_pose_head_forward(ctypes.byref(a), stream) == -1 and b"fc_in" in hip_lib.moss_last_error()
    a.fc_in[22] = 24
    a.parents[5] = 7
    assert hip_lib.moss_pose_head_forward(ctypes.byref(a), stream) == -1 and b"parents" in hip_lib.moss_last_error()


def test_captured_replays_new_frames(gpu, hip_lib):
    """Forward + backward captured ONCE under moss_amd.graphs.capturing (a host synchronisation would fail the capture), replayed over
    four frames whose poses and target_R are copied into the static inputs: every replay is bit-identical to the eager op on that frame."""
    from moss_amd.graphs import capturing
    g = np.load(GOLDEN)
    params, poses, target_R, g_Rs = head_case(g, "trained_large", dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    gen = torch.Generator().manual_seed(5)
    frames = [(poses.clone(), target_R.clone())]
    for _ in range(3):
        axis = 0.4 * torch.randn(23, 3, generator=gen)
        frames.append(((1.2 * torch.rand(1, 72, generator=gen) - 0.6).to(gpu), mlbs.batch_rodrigues(axis).to(gpu)))

    def fn():
        return _run_head(net, poses, target_R, g_Rs)

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, collect=True, stream=side, capture_error_mode="thread_local"):
        outputs = fn()
    torch.cuda.synchronize(gpu)
    first = None
    for k, (p, t) in enumerate(frames):
        poses.copy_(p)
        target_R.copy_(t)
        graph.replay()
        got = [v.clone() for v in outputs]
        torch.cuda.synchronize(gpu)
        ref = fn()
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        if first is None:
            first = got
        else:
            assert not torch.equal(got[0], first[0]) and not torch.equal(got[2], first[2])
    del graph, outputs


class _TinyLbsWeights(torch.nn.Module):
    """A small stand-in for MOSS's cross_attention_lbs: (1,P,3) positions and the (23,3,3) refined rotations -> (1,P,24) offsets."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3 + 23 * 9, 24)

    def forward(self, xyz, Rs):
        x = xyz[0]
        feat = torch.cat([x, Rs.reshape(1, -1).expand(x.shape[0], -1)], 1)
        return 0.2 * self.lin(feat)[None]


def test_renderer_pose_head_in_op(gpu, hip_lib, monkeypatch):
    """render() with pipe.pose_head_in_op on a synthetic body: pose_out["nll"], the image and the gradients of the head's parameters
    agree with the same render() whose head is the torch form (autoregression_torch + matrix_fisher_nll in float64) feeding the same
    fused LBS op -- within twice the single-op bars (two float32 computations): 2 K x the fixture's largest float32 error of nll and
    of a parameter gradient (relative to the gradient's size), and for the image twice the bars tests/test_gpu_lbs.py holds its
    renderer test to (max 2e-3, mean 1e-5: a pixel at the edge of a Gaussian's footprint may flip, the mean may not move).  With the
    flag off, or a pc without the two modules, pose_out and correct_Rs stay None."""
    from moss_amd.gaussian_renderer import render
    from tests.test_gpu_lbs import _pipe, _scene
    g = np.load(GOLDEN)
    s, pc, cam, _ = _scene(gpu)
    params = head_case(g, "trained_small", dtype=torch.float32, device=gpu)[0]
    torch.manual_seed(3)
    poses = cam.smpl_param["poses"]
    cam.smpl_param["pose_rotmats"] = mlbs.batch_rodrigues(poses.reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, device=gpu))
    bg = torch.zeros(3, device=gpu)
    wimg = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    on = _pipe(lbs_in_op=True, pose_head_in_op=True)

    # flag off / modules missing: nothing new runs
    for pipe in (_pipe(lbs_in_op=True), on):
        out = render(cam, pc, pipe, bg)
        assert out["pose_out"] is None and out["correct_Rs"] is None
    pc.auto_regression = _net(params, gpu)
    pc.cross_attention_lbs = _TinyLbsWeights().to(gpu)
    pc.motion_offset_flag = True
    out = render(cam, pc, _pipe(lbs_in_op=True), bg)
    assert out["pose_out"] is None and out["correct_Rs"] is None

    def run():
        for p in pc.auto_regression.parameters():
            p.grad = None
        out = render(cam, pc, on, bg)
        assert out["correct_Rs"].shape == (1, 23, 3, 3) and out["lbs_weights"].shape[2] == 24
        assert out["pose_out"]["target_R"] is cam.smpl_param["pose_rotmats"]
        ((out["render"] * wimg).sum() + 0.06 * out["pose_out"]["nll"].mean()).backward()
        return (out["render"].detach().clone(), out["pose_out"]["nll"].detach().clone(),
                [p.grad.clone() for p in mpose.head_parameters(pc.auto_regression)])

    img, nll, grads = run()

    def head_in_torch(net, poses, target_R, overreg=1.005):
        p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in net.state_dict().items()}
        o = mpose.autoregression_torch(p64, poses.double().cpu())
        n = mpose.matrix_fisher_nll(o["Rs"], o["pose_U"], o["pose_S"], o["pose_V"], target_R.double().cpu(), overreg)
        head_in_torch.leaves = p64
        return {"Rs": o["Rs"].to(gpu).float(), "pose_S": o["pose_S"].detach(), "nll": n.to(gpu).float(), "target_R": target_R}

    monkeypatch.setattr(mpose, "pose_head_fused", head_in_torch)
    out0 = render(cam, pc, on, bg)
    ((out0["render"] * wimg).sum() + 0.06 * out0["pose_out"]["nll"].mean()).backward()
    img0, nll0 = out0["render"].detach(), out0["pose_out"]["nll"].detach()
    assert float(img0.abs().sum()) > 0
    nll_bar = 2 * K * max(float(g[f"{c}_nll_err32"]) for c in HEAD_CASES)
    rel_bar = 2 * K * max(float(g[f"{c}_grad_err32"][i]) / float(np.abs(g[f"{c}_grad_{n}"]).max())
                          for c in HEAD_CASES for i, n in enumerate(mpose.PARAM_NAMES))
    worst = max(float((gr.double().cpu() - head_in_torch.leaves[n].grad).abs().max() / head_in_torch.leaves[n].grad.abs().max())
                for n, gr in zip(mpose.PARAM_NAMES, grads))
    print(f"\nrender with pose_head_in_op vs the torch head: nll {float((nll - nll0).abs().max()):.3g} (bar {nll_bar:.3g}), image max "
          f"{float((img - img0).abs().max()):.3g} mean {float((img - img0).abs().mean()):.3g}, worst relative parameter-gradient "
          f"error {worst:.3g} (bar {rel_bar:.3g})")
    assert float((nll - nll0).abs().max()) < nll_bar
    assert float((img - img0).abs().max()) < 2 * 2e-3 and float((img - img0).abs().mean()) < 2 * 1e-5
    assert worst < rel_bar
