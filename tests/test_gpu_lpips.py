"""The fused LPIPS term on the device (C ABI moss_lpips_vgg_forward / _backward; moss_amd.lpips): the kernels against the reference's own
float64 numbers (tests/golden/lpips_vgg.npz), at a MOSS-sized crop against the torch form on the CPU, the region form, determinism,
every gradient element written, capture in a hipGraph with new inputs per replay, the refusals, and ``evaluate_views(lpips=)``.

The bar (the project's parity factor K = 8, tests/test_gpu_pose.py): float32 against float64 in units of the REFERENCE's own float32
error -- every per-tap term and the total within K x value_err32, the gradient's max-norm error within K x grad_err32_max and its L2
error within K x grad_err32_l2.  ReLU and pool kinks that fall the other way in float32 are in the reference's float32 error too,
which is why the gradient bar is norm-wise; no pixel is excluded.  Nothing here is tuned to the kernels.  Each test prints the worst
ratio of error to err32 it met.
"""
import numpy as np
import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_lpips_cpu import CASES, load_case, run_torch, weights

pytestmark = pytest.mark.gpu

K = 8.0


@pytest.fixture(scope="module")
def net(gpu, hip_lib):
    p = mlp.cast_params(weights(), device=gpu)
    return mlp.LpipsVGG.from_tensors(p["conv_weights"], p["conv_biases"], p["lin_weights"], p["shift"], p["scale"])


def _run(net, x, y):
    """(value (1,1,1,1), terms (5,), dL/dx) of the fused op, detached; the gradient buffer is what autograd hands back."""
    x = x.detach().requires_grad_(True)
    value, terms = mlp.lpips_vgg_fused(net, x, y, return_terms=True)
    (grad,) = torch.autograd.grad(value.sum(), x)
    return value.detach(), terms.detach(), grad.detach()


def _ratios(value, terms, grad, rec):
    """The three ratios error / err32 of a result against a record {terms, total, grad (float64 or float32-rounded), *_err32}."""
    terms64 = terms.double().cpu().numpy()
    verr = max(float(np.abs(terms64 - np.asarray(rec["terms"], dtype=np.float64)).max()),
               abs(float(value.double().cpu().reshape(())) - float(rec["total"])))
    d = grad.double().cpu().numpy().reshape(np.asarray(rec["grad"]).shape) - np.asarray(rec["grad"], dtype=np.float64)
    return {"value": verr / float(rec["value_err32"]), "grad_max": float(np.abs(d).max()) / float(rec["grad_err32_max"]),
            "grad_l2": float(np.sqrt((d * d).sum())) / float(rec["grad_err32_l2"])}


@pytest.mark.parametrize("case", CASES)
def test_matches_reference_float64(gpu, net, case):
    """Each fixture case against the reference's float64 run, within K x its own float32 error; ``same`` is exactly zero."""
    x, y, rec = load_case(case, dtype=torch.float32, device=gpu)
    value, terms, grad = _run(net, x, y)
    assert value.shape == (1, 1, 1, 1) and value.dtype == torch.float32 and grad.shape == x.shape
    if case == "same":
        assert float(value) == 0.0 and not terms.any() and not grad.any()
        return
    r = _ratios(value, terms, grad, rec)
    print(f"lpips {case}: error / err32 = {r}")
    assert max(r.values()) <= K, r


def test_shapes_and_the_forward_that_keeps_nothing(gpu, net):
    """(3,H,W) and (1,3,H,W) give the same bits; the no-grad forward and the forward of an x that needs no gradient equal the
    training forward bit for bit."""
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    v3, t3, g3 = _run(net, x, y)
    v4, t4, g4 = _run(net, x[None], y[None])
    assert g4.shape == (1,) + tuple(x.shape)
    assert torch.equal(v3, v4) and torch.equal(t3, t4) and torch.equal(g3, g4[0])
    with torch.no_grad():
        vn, tn = mlp.lpips_vgg_fused(net, x.clone().requires_grad_(True), y, return_terms=True)
    ve = mlp.lpips_vgg_fused(net, x, y)
    assert not vn.requires_grad and not ve.requires_grad
    assert torch.equal(vn, v3) and torch.equal(tn, t3) and torch.equal(ve, v3)


def test_two_calls_are_bit_identical(gpu, net):
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    a, b = _run(net, x, y), _run(net, x, y)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_every_gradient_element_is_written(gpu, net, hip_lib):
    """The C entry points on a NaN-filled dL_dx, workspace and saved block: the gradient comes back finite everywhere and equal to the
    autograd path's."""
    import ctypes
    from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs, call
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    H, W = x.shape[1:]
    nan_bytes = lambda n: torch.full(((n + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    nws, nsv = hip_lib.moss_lpips_vgg_workspace_bytes(H, W), hip_lib.moss_lpips_vgg_saved_bytes(H, W)
    assert nws > 0 and nsv > 0 and hip_lib.moss_lpips_vgg_saved_bytes(15, 40) == 0
    ws, saved, d_x = nan_bytes(nws), nan_bytes(nsv), torch.full((3, H, W), float("nan"), device=gpu)
    out, g = torch.full((6,), float("nan"), device=gpu), torch.ones(1, device=gpu)
    a = LpipsVggArgs()
    a.x, a.y, a.H, a.W = x.data_ptr(), y.data_ptr(), H, W
    for i in range(13):
        a.weights[i], a.biases[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr()
    for i in range(5):
        a.lin[i] = net.lin[i].data_ptr()
    a.shift, a.scale, a.out, a.terms = net.shift.data_ptr(), net.scale.data_ptr(), out.data_ptr(), out[1:].data_ptr()
    a.saved, a.workspace, a.workspace_bytes = saved.data_ptr(), ws.data_ptr(), nws
    call("moss_lpips_vgg_forward", gpu, ctypes.byref(a))
    ws.fill_(float("nan"))
    b = LpipsVggBackwardArgs()
    b.H, b.W = H, W
    for i in range(13):
        b.weights_bwd[i] = net.w_bwd[i].data_ptr()
    b.scale, b.saved, b.g_out, b.dL_dx = net.scale.data_ptr(), saved.data_ptr(), g.data_ptr(), d_x.data_ptr()
    b.workspace, b.workspace_bytes = ws.data_ptr(), nws
    call("moss_lpips_vgg_backward", gpu, ctypes.byref(b))
    assert bool(torch.isfinite(d_x).all()) and bool(torch.isfinite(out).all())
    value, terms, grad = _run(net, x, y)
    assert torch.equal(d_x, grad) and torch.equal(out[:1], value.reshape(1)) and torch.equal(out[1:], terms)
    a.workspace_bytes = nws - 1
    with pytest.raises(RuntimeError, match="workspace"):
        call("moss_lpips_vgg_forward", gpu, ctypes.byref(a))


def _person_crop(H=256, W=176, seed=7):
    """A crop shaped like MOSS's: a ZJU-MoCap person at 512^2 fills about 256 x 176 -- a smooth figure on a black ground with fine
    texture on it; the render is the ground truth plus blur-like low-frequency error and noise."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    body = np.exp(-(((xx - W / 2) / (0.22 * W)) ** 2 + ((yy - H / 2) / (0.42 * H)) ** 2) ** 2)
    gt = np.stack([body * (0.55 + 0.35 * np.sin(0.11 * xx + 0.07 * yy + c)) + 0.04 * body * rng.standard_normal((H, W)) for c in range(3)])
    low = np.stack([np.sin(0.05 * xx + c) * np.cos(0.04 * yy - c) for c in range(3)])
    x = gt + body * (0.05 * low + 0.03 * rng.standard_normal((3, H, W)))
    return (torch.from_numpy(np.clip(x, 0, 1).astype(np.float32)), torch.from_numpy(np.clip(gt, 0, 1).astype(np.float32)))


def test_person_crop_against_the_torch_form(gpu, net):
    """One crop of MOSS's size, 3 x 256 x 176.  The reference is lpips_vgg_torch on the CPU at test time: float64, and float32 twice
    (contiguous and channels-last) for the three err32 numbers, as the fixture generator measures them.  No torch convolution runs on
    the device."""
    x, y = _person_crop()
    t64, v64, g64 = run_torch(mlp.cast_params(weights(), torch.float64), x.double(), y.double())
    runs = [run_torch(weights(), x, y), run_torch(weights(), x, y, channels_last=True)]
    rec = {"terms": t64.numpy(), "total": float(v64), "grad": g64.numpy(),
           "value_err32": max(max(float((t.double() - t64).abs().max()), abs(float(v) - float(v64))) for t, v, _ in runs),
           "grad_err32_max": max(float((g.double() - g64).abs().max()) for _, _, g in runs),
           "grad_err32_l2": max(float((g.double() - g64).norm()) for _, _, g in runs)}
    assert float(v64) > 1e-6 and rec["value_err32"] > 0 and rec["grad_err32_max"] > 0
    value, terms, grad = _run(net, x.to(gpu), y.to(gpu))
    r = _ratios(value, terms, grad, rec)
    print(f"lpips 256x176: total {float(v64):.6g}, err32 {rec['value_err32']:.3g} / {rec['grad_err32_max']:.3g} / "
          f"{rec['grad_err32_l2']:.3g}, error / err32 = {r}")
    assert max(r.values()) <= K, r


def test_region_form_equals_the_op_on_the_crops(gpu, net):
    """lpips_vgg_roi_fused on a 64 x 64 frame with a 37 x 29 rectangle at an odd offset: the value and the gradient inside the rectangle
    equal lpips_vgg_fused on the two crops bit for bit, and the gradient is zero off the rectangle."""
    from moss_amd.loss import ViewRegion
    gen = torch.Generator().manual_seed(3)
    image, gt = torch.rand(3, 64, 64, generator=gen).to(gpu), torch.rand(3, 64, 64, generator=gen).to(gpu)
    x0, y0, w, h = 13, 21, 37, 29
    mask = torch.zeros(1, 64, 64, device=gpu)
    mask[:, y0:y0 + h, x0:x0 + w] = 1
    region = ViewRegion(mask, rect=(x0, y0, w, h))
    image.requires_grad_(True)
    value, terms = mlp.lpips_vgg_roi_fused(net, image, gt, region, return_terms=True)
    (grad,) = torch.autograd.grad(value.sum(), image)
    cv, ct, cg = _run(net, image.detach()[:, y0:y0 + h, x0:x0 + w], gt[:, y0:y0 + h, x0:x0 + w])
    assert torch.equal(value, cv) and torch.equal(terms, ct)
    assert torch.equal(grad[:, y0:y0 + h, x0:x0 + w], cg) and bool(cg.any())
    off = grad.clone()
    off[:, y0:y0 + h, x0:x0 + w] = 0
    assert not off.any()


def test_capture_and_replay_with_new_inputs(gpu, net):
    """Forward + backward captured ONCE under moss_amd.graphs.capturing (a host synchronisation would fail the capture), replayed with
    new images copied into the static inputs: every replay is bit-identical to the eager op on those inputs."""
    from moss_amd.graphs import capturing
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    gen = torch.Generator().manual_seed(9)
    frames = [(x.clone(), y.clone())] + [(torch.rand(x.shape, generator=gen).to(gpu), torch.rand(x.shape, generator=gen).to(gpu))
                                          for _ in range(2)]

    def fn():
        return _run(net, x, y)

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
    seen = []
    for k, (fx, fy) in enumerate(frames):
        x.copy_(fx)
        y.copy_(fy)
        graph.replay()
        got = [v.clone() for v in outputs]
        torch.cuda.synchronize(gpu)
        ref = fn()
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), (k, i)
        seen.append(float(got[0]))
    assert len(set(seen)) == len(frames)


def test_refusals(gpu, net):
    x, y, _ = load_case("min", dtype=torch.float32, device=gpu)
    with pytest.raises(RuntimeError, match="gets no gradient"):
        mlp.lpips_vgg_fused(net, x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="batch must be 1"):
        mlp.lpips_vgg_fused(net, torch.stack([x, x]), torch.stack([y, y]))
    with pytest.raises(ValueError, match=">= 16"):
        mlp.lpips_vgg_fused(net, x[:, :15], y[:, :15])
    with pytest.raises(RuntimeError, match="on a GPU"):
        mlp.lpips_vgg_fused(net, x.cpu(), y.cpu())
    with pytest.raises(ValueError, match="float32"):
        mlp.lpips_vgg_fused(net, x.double(), y.double())


def test_evaluate_views_adds_lpips(gpu, net):
    """evaluate_views(..., lpips=net) on three 32 x 32 views: the LPIPS mean is the float64 sum, in view order, of three single calls of
    the fused op on the images the split driver hands its LPIPS, over 3; the other keys are what they are without ``lpips=``."""
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import evaluate_views
    scene = scenes.config2()
    c0 = scene.camera
    s = 32.0 / c0.W
    cams = [camera_view(scenes.make_camera(32, 32, float(c0.K[0, 0]) * s, float(c0.K[1, 1]) * s, 16.0, 16.0, R, t), gpu)
            for R, t in scenes.look_at_ring(3)]
    pc = GaussianSet(scene, sh_degree=3, device=gpu, unified_features=True)
    bg = torch.zeros(3, device=gpu)
    gen = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, 32, 32, generator=gen).to(gpu) for _ in range(3)]
    mask = torch.zeros(1, 32, 32, device=gpu)
    mask[:, 4:30, 3:27] = 1
    regions = [ViewRegion(mask), None, ViewRegion(mask)]
    plain = evaluate_views(pc, cams, gts, regions, bg)
    pairs = []
    evaluate_views(pc, cams, gts, regions, bg, lpips_fn=lambda a, b: (pairs.append((a.clone(), b.clone())), a.sum() * 0)[1])
    got = evaluate_views(pc, cams, gts, regions, bg, lpips=net)
    assert len(pairs) == 3 and plain["lpips"] is None
    for k in ("l1", "psnr", "ssim", "n"):
        assert got[k] == plain[k], k
    total = torch.zeros((), dtype=torch.float64, device=gpu)
    for a, b in pairs:
        total += mlp.lpips_vgg_fused(net, a, b).mean().double()
    assert got["lpips"] == float(total) / 3 and got["lpips"] > 0
    with pytest.raises(ValueError, match="not both"):
        evaluate_views(pc, cams, gts, regions, bg, lpips=net, lpips_fn=lambda a, b: a.sum())
