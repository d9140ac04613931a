"""The split-bf16 (three-product) mode of the fused LBS-weight network on the device (C ABI moss_lbs_weight_net_forward_bf16x3 /
_backward_bf16x3; cross_attention_lbs_fused(precision="bf16x3")): the kernels against the exact float64 statement of their own
arithmetic (cross_attention_lbs_torch(operand_dtype=torch.bfloat16, operand_split=True) in float64), tails, the distance from the exact
network against what bf16 operands could reach, structure (determinism, every element written, shapes, no_grad), the modes apart,
gradient sinks, capture in a hipGraph, MOSS's size, render() and MossStep.

The bars.  tests/test_lbs_weights_bf16x3_cpu.py builds the cases (points away from every ReLU kink of the float64 split form) and,
beside every float64 result X of the split form, err32_form[X]: what the same form loses when it runs in float32.  A kernel result may
be off by K = 8 times that (the project's parity factor, imported from tests/test_gpu_lbs_weights.py).  Nothing here is tuned to the
kernels; every test prints the figures it met.
"""
import ctypes

import pytest
import torch

from moss_amd import lbs_weights as mlw
from tests.test_gpu_lbs_weights import K, _net, _random_inputs
from tests.test_gpu_moss_step import LRS, _fresh, _load, _release_device_memory, _state, world  # noqa: F401  (fixtures of that module, by import)
from tests.test_lbs_weights_bf16x3_cpu import QUANTITIES, ROUNDED, SPLIT, build_case, form_on
from tests.test_lbs_weights_cpu import CASES, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_blas_workspaces():
    """As tests/test_gpu_lbs_weights.py: the torch yardsticks' BLAS workspaces are released after every test."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch._C._cuda_clearCublasWorkspaces()


def _run(net, x, Rs, cot, precision="bf16x3", **kw):
    """out and the 18 gradients of <out, cot> (x, Rs, the 16 parameters), detached, in QUANTITIES order."""
    x = x.detach().requires_grad_(True)
    Rs = Rs.detach().requires_grad_(True)
    out = mlw.cross_attention_lbs_fused(net, x[None], Rs, precision=precision, **kw)
    grads = torch.autograd.grad((out * cot).sum(), [x, Rs] + mlw.net_parameters(net))
    return [out.detach()] + [v.detach() for v in grads]


def _case_on(case, gpu, P=None):
    """(net, x, Rs, cot on the device, the built case) -- the first P points of the case, or all."""
    c = build_case(case)
    n = c["x"].shape[0] if P is None else P
    net = _net({k: v.float() for k, v in c["params"].items()}, gpu)
    return net, c["x"][:n].to(gpu), c["Rs"].to(gpu), c["cot"][:, :n].contiguous().to(gpu), c


def _ratios(got, ref64, err32):
    return {k: float((v.double().cpu() - ref64[k]).abs().max()) / err32[k] for k, v in zip(QUANTITIES, got)}


@pytest.mark.parametrize("case", CASES)
def test_kernels_compute_the_split_form(gpu, hip_lib, case):
    """out and all 18 gradients against the float64 split form on the built case, each within K x its err32_form; out_layer /
    gate_proj get no gradient."""
    net, x, Rs, cot, c = _case_on(case, gpu)
    x.requires_grad_(True)
    Rs.requires_grad_(True)
    out = mlw.cross_attention_lbs_fused(net, x[None], Rs, precision="bf16x3")
    assert out.shape == (1, x.shape[0], 24) and out.dtype == torch.float32
    (out * cot).sum().backward()
    named = dict(net.named_parameters())
    got = [out.detach(), x.grad, Rs.grad] + [named[k].grad for k in mlw.PARAM_NAMES]
    for k, v in zip(QUANTITIES, got):
        assert v is not None and v.shape == c["form64"][k].shape, k
    ratios = _ratios(got, c["form64"], c["err32_form"])
    worst = max(ratios, key=ratios.get)
    print(f"\n{case}: error / err32_form: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" (worst: {worst})")
    assert ratios[worst] < K, ratios
    for k in mlw.UNUSED_NAMES:
        assert named[k].grad is None, k


@pytest.mark.parametrize("P", [1, 31, 33, 65])
def test_tails(gpu, hip_lib, P):
    """The first P points of the sharp case (their kink clearance is the case's): out and the gradients against the split form run on
    exactly those points, each within K x that run's err32_form."""
    net, x, Rs, cot, c = _case_on("sharp", gpu, P)
    f64, err32 = form_on("sharp", c["x"][:P], c["Rs"], c["cot"][:, :P])
    ratios = _ratios(_run(net, x, Rs, cot), f64, err32)
    worst = max(ratios, key=ratios.get)
    print(f"\nP = {P}: error / err32_form: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" (worst: {worst})")
    assert ratios[worst] < K, ratios


@pytest.mark.parametrize("case", CASES)
def test_closer_to_float64_than_bf16_operands_can_be(gpu, hip_lib, case):
    """The kernel's out and g_x are closer to the exact float64 network than the float64 rounded-bf16 form is."""
    net, x, Rs, cot, c = _case_on(case, gpu)
    got = dict(zip(QUANTITIES, _run(net, x, Rs, cot)))
    for k in ("out", "x"):
        d_kernel = float((got[k].double().cpu() - c["exact64"][k]).abs().max())
        d_round = float((c["rounded64"][k] - c["exact64"][k]).abs().max())
        print(f"\n{case} {k}: distance from the exact float64 network: kernel {d_kernel:.3g}, rounded-bf16 form {d_round:.3g} "
              f"({d_round / d_kernel:.0f} x)")
        assert d_kernel < d_round, k


def test_structure(gpu, hip_lib):
    """Two calls are bit-identical; (1,P,3) / (P,3) and (23,3,3) / (1,23,3,3) give the same bits; under no_grad the forward keeps
    nothing and returns the same values.  Through the C ABI with out, saved, g_x, g_Rs, the workspace and the 16 gradient buffers
    pre-filled with NaN, none is left in an output; a zero cotangent gives all-zero gradients; P = 0 succeeds; a short workspace is
    refused."""
    from moss_amd._lib import LbsWeightNetArgs, LbsWeightNetBackwardArgs, check
    net, x, Rs, cot, c = _case_on("init", gpu)
    a = [v.clone() for v in _run(net, x, Rs, cot)]
    b = _run(net, x, Rs, cot)
    assert len(a) == 19
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v) and bool(u.any()), i
    with torch.no_grad():
        assert torch.equal(mlw.cross_attention_lbs_fused(net, x, Rs[None], precision="bf16x3"), a[0])
    res = _run(net, x[:0], Rs, cot[:, :0])
    assert res[0].shape == (1, 0, 24) and res[1].shape == (0, 3) and not any(bool(v.any()) for v in res)

    plist = [p.detach().contiguous() for p in mlw.net_parameters(net)]
    P = int(x.shape[0])
    nan = float("nan")
    out = torch.full((P, 24), nan, device=gpu)
    saved = torch.full((hip_lib.moss_lbs_weight_net_saved_bytes(P) // 4,), nan, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    fa = LbsWeightNetArgs()
    fa.P, fa.x, fa.Rs, fa.out, fa.saved = P, x.data_ptr(), Rs.data_ptr(), out.data_ptr(), saved.data_ptr()
    for i, p in enumerate(plist):
        fa.params[i] = p.data_ptr()
    check(hip_lib.moss_lbs_weight_net_forward_bf16x3(ctypes.byref(fa), stream), "forward")
    torch.cuda.synchronize(gpu)
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(saved).any())
    assert torch.equal(out, a[0][0])
    nbytes = hip_lib.moss_lbs_weight_net_workspace_bytes(P)
    for cotangent in (cot.reshape(P, 24).contiguous(), torch.zeros(P, 24, device=gpu)):
        ws = torch.full((nbytes // 4,), nan, device=gpu)
        g_x, g_Rs = torch.full((P, 3), nan, device=gpu), torch.full((23, 3, 3), nan, device=gpu)
        grads = [torch.full_like(p, nan) for p in plist]
        ba = LbsWeightNetBackwardArgs()
        ba.P, ba.Rs, ba.saved, ba.g_out, ba.g_x, ba.g_Rs = P, Rs.data_ptr(), saved.data_ptr(), cotangent.data_ptr(), g_x.data_ptr(), g_Rs.data_ptr()
        ba.workspace, ba.workspace_bytes = ws.data_ptr(), nbytes
        for i, (p, t) in enumerate(zip(plist, grads)):
            ba.params[i], ba.grads[i] = p.data_ptr(), t.data_ptr()
        check(hip_lib.moss_lbs_weight_net_backward_bf16x3(ctypes.byref(ba), stream), "backward")
        torch.cuda.synchronize(gpu)
        for name, t in zip(QUANTITIES[1:], [g_x, g_Rs] + grads):
            assert not bool(torch.isnan(t).any()), name
            assert bool(t.any()) == bool(cotangent.any()), name
        if bool(cotangent.any()):
            for name, t, ref in zip(QUANTITIES[1:], [g_x, g_Rs] + grads, a[1:]):
                assert torch.equal(t.reshape(ref.shape), ref), name
    ba.workspace_bytes = nbytes - 1
    assert hip_lib.moss_lbs_weight_net_backward_bf16x3(ctypes.byref(ba), stream) == -1
    assert b"moss_lbs_weight_net_backward_bf16x3: the workspace" in hip_lib.moss_last_error()
    ba.workspace_bytes = nbytes
    ba.grads[15] = None
    assert hip_lib.moss_lbs_weight_net_backward_bf16x3(ctypes.byref(ba), stream) == -1 and b"16" in hip_lib.moss_last_error()
    fa.P = ba.P = 0
    assert hip_lib.moss_lbs_weight_net_forward_bf16x3(ctypes.byref(fa), stream) == 0
    assert hip_lib.moss_lbs_weight_net_backward_bf16x3(ctypes.byref(ba), stream) == 0


def test_modes_are_distinct_and_the_default_untouched(gpu, hip_lib):
    """precision="f32" equals the call without the argument bit for bit (out and all gradients); "bf16x3" differs from it somewhere
    in out."""
    net, x, Rs, cot, c = _case_on("sharp", gpu)
    xr, Rr = x.detach().requires_grad_(True), Rs.detach().requires_grad_(True)
    out = mlw.cross_attention_lbs_fused(net, xr[None], Rr)
    plain = [out.detach()] + list(torch.autograd.grad((out * cot).sum(), [xr, Rr] + mlw.net_parameters(net)))
    f32 = _run(net, x, Rs, cot, precision="f32")
    for i, (u, v) in enumerate(zip(plain, f32)):
        assert torch.equal(u, v), i
    split = _run(net, x, Rs, cot)
    diff = float((split[0] - f32[0]).abs().max())
    print(f"\nout: bf16x3 against f32, largest difference {diff:.3g}")
    assert not torch.equal(split[0], f32[0])
    with pytest.raises(ValueError, match="precision must be one of"):
        mlw.cross_attention_lbs_fused(net, x[None], Rs, precision="bf16")


def test_grad_sink(gpu, hip_lib):
    """With a sink per parameter the 16 gradients land in the sinks (autograd receives those tensors), bit-equal to the run without."""
    net, x, Rs, cot, c = _case_on("init", gpu)
    ref = [v.clone() for v in _run(net, x, Rs, cot)]
    params = mlw.net_parameters(net)
    sinks = {id(p): torch.full_like(p, float("nan")) for p in params}
    got = _run(net, x, Rs, cot, grad_sink=lambda p: sinks[id(p)])
    for i, (u, v) in enumerate(zip(got, ref)):
        assert torch.equal(u, v), i
    for p, g, r in zip(params, got[3:], ref[3:]):
        assert g.data_ptr() == sinks[id(p)].data_ptr() and torch.equal(sinks[id(p)], r)


def test_captured_replays_new_inputs(gpu, hip_lib):
    """Forward + backward captured once, replayed with new x / Rs copied into the static inputs: every replay is bit-identical to the
    eager op on those inputs."""
    from moss_amd.graphs import capturing
    net, x, Rs, cot, c = _case_on("sharp", gpu)
    P = int(x.shape[0])
    frames = [(x.clone(), Rs.clone())] + [_random_inputs(P, gpu, 60 + i)[:2] for i in range(3)]

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


def test_moss_size(gpu, hip_lib):
    """P = 45 695, random inputs, the sharp parameters: out against the float64 split form on the device within K x the float32 split
    form's own error there; the gradients finite and bit-identical between two calls."""
    P = 45695
    params = load_case("sharp", dtype=torch.float32, device=gpu)[1]
    net = _net(params, gpu)
    x, Rs, cot = _random_inputs(P, gpu, 7 + P)
    a = [v.clone() for v in _run(net, x, Rs, cot)]
    with torch.no_grad():
        ref64 = mlw.cross_attention_lbs_torch({k: v.double() for k, v in params.items()}, x.double(), Rs.double(), **SPLIT)
        ref32 = mlw.cross_attention_lbs_torch(params, x, Rs, **SPLIT)
        bar = K * (ref32.double() - ref64).abs().max()
        err = (a[0].double() - ref64).abs().max()
    print(f"\nP = {P}: out error {float(err):.3g}, bar {float(bar):.3g} (K x the float32 split form's error)")
    assert float(err) < float(bar)
    assert len(a) == 19
    for i, (u, v) in enumerate(zip(a, _run(net, x, Rs, cot))):
        assert bool(torch.isfinite(u).all()), i
        assert torch.equal(u, v), i


def test_renderer_lbs_weights_precision(gpu, hip_lib):
    """render() with pipe.lbs_weights_in_op and pipe.lbs_weights_precision="bf16x3" against the same render in f32 mode: the image
    within the bars of tests/test_gpu_lbs_weights.py's render test (max 2e-3, mean 1e-5); lbs_weights within K x the difference the
    float64 split form shows against the exact float64 network on the same inputs, carried through the skinning softmax
    (softmax(log(W + 1e-9) + offsets)) on the CPU."""
    from moss_amd import lbs as mlbs
    from moss_amd import pose as mpose
    from moss_amd.gaussian_renderer import render
    from tests.test_gpu_lbs import _pipe, _scene
    s, pc, cam, _ = _scene(gpu)
    params = load_case("sharp", dtype=torch.float32, device=gpu)[1]
    torch.manual_seed(3)
    poses = cam.smpl_param["poses"]
    cam.smpl_param["pose_rotmats"] = mlbs.batch_rodrigues(poses.reshape(24, 3)[1:] + 0.05 * torch.randn(23, 3, device=gpu))
    bg = torch.zeros(3, device=gpu)
    pc.auto_regression = mpose.head_module().to(gpu)
    pc.cross_attention_lbs = _net(params, gpu)
    pc.motion_offset_flag = True

    def run(**kw):
        with torch.no_grad():
            out = render(cam, pc, _pipe(lbs_in_op=True, pose_head_in_op=True, lbs_weights_in_op=True, **kw), bg)
        return out["render"].clone(), out["lbs_weights"].clone(), out["pose_out"]["Rs"].clone()

    img0, w0, Rs = run()
    img1, w1, _ = run(lbs_weights_precision="f32")
    assert torch.equal(img0, img1) and torch.equal(w0, w1)                       # (the flag's default is the f32 mode)
    img, w, _ = run(lbs_weights_precision="bf16x3")
    assert float(img0.abs().sum()) > 0 and not torch.equal(w, w0)
    # the bar, measured: the two float64 forms on the render's own inputs, through the skinning softmax
    xyz = pc.get_xyz.detach()
    _, ids = pc.knn(cam.big_pose_world_vertex[None].float(), xyz[None].float())
    base = torch.log(pc.SMPL_NEUTRAL["weights"][ids.reshape(-1)].double().cpu() + 1e-9)
    p64 = {k: v.double().cpu() for k, v in params.items()}
    with torch.no_grad():
        off_exact = mlw.cross_attention_lbs_torch(p64, xyz.double().cpu(), Rs.double().cpu())[0]
        off_split = mlw.cross_attention_lbs_torch(p64, xyz.double().cpu(), Rs.double().cpu(), **SPLIT)[0]
    form_diff = float((torch.softmax(base + off_split, -1) - torch.softmax(base + off_exact, -1)).abs().max())
    w_bar = K * form_diff
    d_img, d_w = (img - img0).abs(), float((w - w0).abs().max())
    print(f"\nrender, bf16x3 against f32 mode: image max {float(d_img.max()):.3g} mean {float(d_img.mean()):.3g}; lbs_weights {d_w:.3g} "
          f"(bar {w_bar:.3g} = K x {form_diff:.3g}, the float64 split form against the exact network)")
    assert float(d_img.max()) < 2e-3 and float(d_img.mean()) < 1e-5
    assert d_w < w_bar


def test_moss_step_with_bf16x3_lbs_weights(gpu, hip_lib, world):
    """tests/test_gpu_moss_step.py's world with MossStep(lbs_weights_precision="bf16x3"): one eager step and one replayed step agree
    bit for bit (terms, render, every parameter and moment); all seven terms are finite; the step differs from the f32 step."""
    from moss_amd.train import MossStep

    def step(**kw):
        pc, cam, _ = _fresh(world)
        return MossStep(pc, cam, world["gt"], world["bkgd"], world["region"], world["bg"], world["lpips"], LRS, **kw), cam

    (eager, ce), (graphed, cg), (plain, cp) = step(lbs_weights_precision="bf16x3"), step(lbs_weights_precision="bf16x3"), step()
    assert eager.pipe.lbs_weights_precision == "bf16x3" and plain.pipe.lbs_weights_precision == "f32"
    graphed.capture(warmup=3)
    for cam in (ce, cg, cp):
        _load(cam, 1, gpu)
    out_e = eager.compute()
    te, ie = out_e["terms"].clone(), out_e["render"].clone()
    out_g = graphed()
    tg, ig = out_g["terms"].clone(), out_g["render"].clone()
    out_p = plain.compute()
    tp = out_p["terms"].clone()
    torch.cuda.synchronize(gpu)
    print(f"\nterms: bf16x3 {te.tolist()}, f32 {tp.tolist()}")
    assert te.shape == (7,) and bool(torch.isfinite(te).all())
    assert torch.equal(te, tg), (te.tolist(), tg.tolist())
    assert torch.equal(ie, ig)
    for i, (u, v) in enumerate(zip(_state(eager), _state(graphed))):
        assert torch.equal(u, v), i
    graphed.check()
    assert graphed.dropped_frames == 0
    assert any(not torch.equal(u, v) for u, v in zip(_state(eager), _state(plain)))
    with pytest.raises(ValueError, match="lbs_weights_precision must be one of"):
        step(lbs_weights_precision="bf16")
