"""The fused LBS-weight network on the device (C ABI moss_lbs_weight_net_forward / _backward; moss_amd.lbs_weights): the kernels
against the reference's own float64 numbers (tests/golden/lbs_weights_*.npz), at MOSS's sizes against the torch form in float64,
determinism, every gradient written, capture in a hipGraph with new inputs per replay, and the renderer's ``pipe.lbs_weights_in_op``.

The bars.  Beside every float64 result X the fixtures store X_err32: what the REFERENCE loses when it runs in float32 on the same
inputs.  A kernel result may be off by K = 8 times that (the project's parity factor, tests/test_gpu_pose.py: a float32 computation
with another summation order, no better and no worse than the reference's own).  Nothing here is tuned to the kernels.  The
fixtures' points keep away from every ReLU kink (tests/golden/make_golden_lbs_weights.py); no point is excluded here.  Each test
prints the worst ratio of error to err32 it met.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from moss_amd import lbs_weights as mlw
from tests.test_lbs_weights_cpu import CASES, GOLDEN_DIR, GRAD_NAMES, load_case

pytestmark = pytest.mark.gpu

K = 8.0


@pytest.fixture(autouse=True)
def _release_blas_workspaces():
    """The torch yardsticks of this file run GEMMs on the device, and torch keeps a BLAS workspace per handle alive for the rest of the
    process (0.2 GiB each, counted as allocated memory).  They are released after every test here, so that a later test that bounds
    the process's peak memory sees what it saw without this file."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch._C._cuda_clearCublasWorkspaces()


def _net(params, dev):
    net = mlw.lbs_weight_module()
    net.load_state_dict({k: v.float() for k, v in params.items()})
    return net.to(dev)


def _err(got, ref):
    return float(np.abs(got.detach().double().cpu().numpy() - np.asarray(ref, dtype=np.float64)).max())


def _run(net, x, Rs, cot):
    """out and the 18 gradients of <out, cot> (x, Rs, the 16 parameters), detached."""
    x = x.detach().requires_grad_(True)
    Rs = Rs.detach().requires_grad_(True)
    out = mlw.cross_attention_lbs_fused(net, x[None], Rs)
    grads = torch.autograd.grad((out * cot).sum(), [x, Rs] + mlw.net_parameters(net))
    return [out.detach()] + [v.detach() for v in grads]


def _random_inputs(P, dev, seed):
    from moss_amd import lbs as mlbs
    gen = torch.Generator().manual_seed(seed)
    x = (2 * torch.rand(P, 3, generator=gen) - 1).to(dev)
    Rs = mlbs.batch_rodrigues(0.4 * torch.randn(23, 3, generator=gen)).to(dev)
    cot = torch.randn(1, P, 24, generator=gen).to(dev)
    return x, Rs, cot


@pytest.mark.parametrize("case", CASES)
def test_matches_reference_float64(gpu, hip_lib, case):
    """cross_attention_lbs_fused: out and the gradient of <out, g> w.r.t. x, Rs and each of the 16 parameters against the reference's
    float64 run, each within K x the reference's own float32 error of that quantity; out_layer / gate_proj get no gradient."""
    g, params, x, Rs, cot = load_case(case, dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    x.requires_grad_(True)
    Rs.requires_grad_(True)
    out = mlw.cross_attention_lbs_fused(net, x[None], Rs)
    assert out.shape == (1, x.shape[0], 24) and out.dtype == torch.float32
    (out * cot).sum().backward()
    named = dict(net.named_parameters())
    got = {"x": x.grad, "Rs": Rs.grad, **{k: named[k].grad for k in mlw.PARAM_NAMES}}
    ratios = {"out": _err(out, g["out"]) / float(g["out_err32"])}
    for k in GRAD_NAMES:
        assert got[k] is not None and got[k].shape == g[f"grad_{k}"].shape, k
        ratios[k] = _err(got[k], g[f"grad_{k}"]) / float(g[f"grad_{k}_err32"])
    worst = max(ratios, key=ratios.get)
    print(f"\n{case}: error / err32: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" (worst: {worst})")
    assert ratios[worst] < K, ratios
    for k in mlw.UNUSED_NAMES:
        assert named[k].grad is None, k
    # (1,P,3) / (P,3) and (23,3,3) / (1,23,3,3): the same bits; without a gradient the same values from the forward that keeps nothing
    with torch.no_grad():
        assert torch.equal(mlw.cross_attention_lbs_fused(net, x.detach(), Rs.detach()[None]), out.detach())


@pytest.mark.parametrize("P", [45695, 100000])
def test_moss_sizes(gpu, hip_lib, P):
    """At MOSS's size and the bench frame's, random inputs: out against cross_attention_lbs_torch in float64 on the device, within K x
    the error of the same torch form in float32 on the same inputs (the torch form is pinned to the reference by the CPU test; out is
    continuous across a ReLU kink, so no point is left out).  Gradients: finite and bit-identical between two calls (kinks are not
    controlled at this size)."""
    params = load_case("sharp", dtype=torch.float32, device=gpu)[1]
    net = _net(params, gpu)
    x, Rs, cot = _random_inputs(P, gpu, 7 + P)
    a = [v.clone() for v in _run(net, x, Rs, cot)]
    with torch.no_grad():
        ref64 = mlw.cross_attention_lbs_torch({k: v.double() for k, v in params.items()}, x.double(), Rs.double())
        ref32 = mlw.cross_attention_lbs_torch(params, x, Rs)
        bar = K * (ref32.double() - ref64).abs().max()
        err = (a[0].double() - ref64).abs().max()
    print(f"\nP = {P}: out error {float(err):.3g}, bar {float(bar):.3g} (K x the float32 torch form's error)")
    assert float(err) < float(bar)
    assert len(a) == 19
    for i, v in enumerate(a):
        assert bool(torch.isfinite(v).all()), i
    if P == 45695:
        for i, (u, v) in enumerate(zip(a, _run(net, x, Rs, cot))):
            assert torch.equal(u, v), i


def test_deterministic(gpu, hip_lib):
    """Two calls on the same inputs: bit-identical out and all 18 gradients (a fixture size; 45 695 is in test_moss_sizes)."""
    g, params, x, Rs, cot = load_case("init", dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    a = [v.clone() for v in _run(net, x, Rs, cot)]
    b = _run(net, x, Rs, cot)
    assert len(a) == 19
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
        assert bool(u.any()), i


def test_every_gradient_is_written(gpu, hip_lib):
    """Through the C ABI: out, saved, g_x, g_Rs, the workspace and the 16 gradient buffers are pre-filled with NaN; the forward and
    the backward leave none in their outputs (they write, never accumulate).  A zero cotangent gives all-zero gradients.  P = 0
    succeeds.  A short workspace is refused."""
    from moss_amd._lib import LbsWeightNetArgs, LbsWeightNetBackwardArgs, check
    g, params, x, Rs, cot = load_case("init", dtype=torch.float32, device=gpu)
    plist = [params[k].contiguous() for k in mlw.PARAM_NAMES]
    P = int(x.shape[0])
    nan = float("nan")
    out = torch.full((P, 24), nan, device=gpu)
    saved = torch.full((hip_lib.moss_lbs_weight_net_saved_bytes(P) // 4,), nan, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    a = LbsWeightNetArgs()
    a.P, a.x, a.Rs, a.out, a.saved = P, x.data_ptr(), Rs.data_ptr(), out.data_ptr(), saved.data_ptr()
    for i, p in enumerate(plist):
        a.params[i] = p.data_ptr()
    check(hip_lib.moss_lbs_weight_net_forward(ctypes.byref(a), stream), "forward")
    torch.cuda.synchronize(gpu)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(saved).any())
    nbytes = hip_lib.moss_lbs_weight_net_workspace_bytes(P)
    for cotangent in (cot.reshape(P, 24).contiguous(), torch.zeros(P, 24, device=gpu)):
        ws = torch.full((nbytes // 4,), nan, device=gpu)
        g_x, g_Rs = torch.full((P, 3), nan, device=gpu), torch.full((23, 3, 3), nan, device=gpu)
        grads = [torch.full_like(p, nan) for p in plist]
        b = LbsWeightNetBackwardArgs()
        b.P, b.Rs, b.saved, b.g_out, b.g_x, b.g_Rs = P, Rs.data_ptr(), saved.data_ptr(), cotangent.data_ptr(), g_x.data_ptr(), g_Rs.data_ptr()
        b.workspace, b.workspace_bytes = ws.data_ptr(), nbytes
        for i, (p, t) in enumerate(zip(plist, grads)):
            b.params[i], b.grads[i] = p.data_ptr(), t.data_ptr()
        check(hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), stream), "backward")
        torch.cuda.synchronize(gpu)
        for name, t in zip(GRAD_NAMES, [g_x, g_Rs] + grads):
            assert not bool(torch.isnan(t).any()), name
            assert bool(t.any()) == bool(cotangent.any()), name
    b.workspace_bytes = nbytes - 1
    assert hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), stream) == -1 and b"workspace" in hip_lib.moss_last_error()
    b.workspace_bytes = nbytes
    b.grads[15] = None
    assert hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), stream) == -1 and b"16" in hip_lib.moss_last_error()
    a.P = 0
    assert hip_lib.moss_lbs_weight_net_forward(ctypes.byref(a), stream) == 0
    b.P = 0
    assert hip_lib.moss_lbs_weight_net_backward(ctypes.byref(b), stream) == 0
    # P = 0 through the Python op: an empty output and zero gradients
    net = _net(params, gpu)
    res = _run(net, x[:0], Rs, cot[:, :0])
    assert res[0].shape == (1, 0, 24) and res[1].shape == (0, 3) and not any(bool(v.any()) for v in res)


def test_captured_replays_new_inputs(gpu, hip_lib):
    """Forward + backward captured ONCE under moss_amd.graphs.capturing (a host synchronisation would fail the capture), replayed with
    new x / Rs copied into the static inputs: every replay is bit-identical to the eager op on those inputs."""
    from moss_amd.graphs import capturing
    g, params, x, Rs, cot = load_case("sharp", dtype=torch.float32, device=gpu)
    net = _net(params, gpu)
    P = int(x.shape[0])
    frames = [(x.clone(), Rs.clone())] + [_random_inputs(P, gpu, 40 + i)[:2] for i in range(3)]

    def fn():
        return _run(net, x, Rs, cot)

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
    for k, (fx, fR) in enumerate(frames):
        x.copy_(fx)
        Rs.copy_(fR)
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


def test_renderer_lbs_weights_in_op(gpu, hip_lib):
    """render() with pipe.pose_head_in_op + pipe.lbs_weights_in_op and pc.cross_attention_lbs = lbs_weight_module() against the same
    render() with lbs_weights_in_op off (the module's own torch forward): the image within the bars tests/test_gpu_lbs.py holds its
    renderer test to (max 2e-3, mean 1e-5), the lbs_weights output (the softmax of log W + offsets: it does not amplify an offset
    error) within 2 K x the fixtures' largest out_err32 (two float32 computations); the gradients of the network's parameters and of
    _xyz finite and nonzero.  With the flag set and a module of another layout render() raises."""
    from moss_amd import lbs as mlbs
    from moss_amd import pose as mpose
    from moss_amd.gaussian_renderer import render
    from tests.test_gpu_lbs import _pipe, _scene
    from tests.test_gpu_pose import _TinyLbsWeights
    s, pc, cam, _ = _scene(gpu)
    params = load_case("sharp", dtype=torch.float32, device=gpu)[1]
    torch.manual_seed(3)
    poses = cam.smpl_param["poses"]
    cam.smpl_param["pose_rotmats"] = mlbs.batch_rodrigues(poses.reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, device=gpu))
    bg = torch.zeros(3, device=gpu)
    wimg = torch.rand(3, s.camera.H, s.camera.W, device=gpu)
    pc.auto_regression = mpose.head_module().to(gpu)
    pc.cross_attention_lbs = _net(params, gpu)
    pc.motion_offset_flag = True
    xyz = pc._xyz
    if not xyz.requires_grad:
        xyz.requires_grad_(True)

    def run(pipe):
        for p in list(pc.cross_attention_lbs.parameters()) + [xyz]:
            p.grad = None
        out = render(cam, pc, pipe, bg)
        (out["render"] * wimg).sum().backward()
        return out["render"].detach().clone(), out["lbs_weights"].detach().clone()

    img0, w0 = run(_pipe(lbs_in_op=True, pose_head_in_op=True))
    on = _pipe(lbs_in_op=True, pose_head_in_op=True, lbs_weights_in_op=True)
    img, w = run(on)
    assert float(img0.abs().sum()) > 0
    named = dict(pc.cross_attention_lbs.named_parameters())
    for k in mlw.PARAM_NAMES:
        assert named[k].grad is not None and bool(torch.isfinite(named[k].grad).all()) and bool(named[k].grad.any()), k
    for k in mlw.UNUSED_NAMES:
        assert named[k].grad is None, k
    assert bool(torch.isfinite(xyz.grad).all()) and bool(xyz.grad.any())
    w_bar = 2 * K * max(float(np.load(os.path.join(GOLDEN_DIR, f"lbs_weights_{c}.npz"))["out_err32"]) for c in CASES)
    print(f"\nrender with lbs_weights_in_op vs the module's torch forward: image max {float((img - img0).abs().max()):.3g} mean "
          f"{float((img - img0).abs().mean()):.3g}, lbs_weights {float((w - w0).abs().max()):.3g} (bar {w_bar:.3g})")
    assert float((img - img0).abs().max()) < 2e-3 and float((img - img0).abs().mean()) < 1e-5
    assert float((w - w0).abs().max()) < w_bar
    # a module of another layout: no fallback
    pc.cross_attention_lbs = _TinyLbsWeights().to(gpu)
    with pytest.raises(ValueError, match="bw_linears"):
        render(cam, pc, on, bg)
    render(cam, pc, _pipe(lbs_in_op=True, pose_head_in_op=True), bg)          # flag off: the stand-in runs as before
