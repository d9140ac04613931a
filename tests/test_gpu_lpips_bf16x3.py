"""The split-bf16 (three-product) mode of the fused LPIPS term on the device (``LpipsVGG(precision="bf16x3")``; C ABI
``moss_lpips_vgg_forward_bf16x3`` / ``_backward_bf16x3`` / ``_pack_weights_bf16x3``, conv3x3_bf16x3_kernel of csrc/lpips.hip).  It mirrors
tests/test_gpu_lpips_bf16.py.

1. The kernels compute what they claim: against ``lpips_vgg_torch(..., operand_dtype=torch.bfloat16, operand_split=True)`` in float64 on
   the CPU -- the exact statement of the arithmetic -- within K = 8 of err32, the largest error of four float32 CPU runs of that same
   form (tests/test_lpips_bf16x3_cpu.py measures them and checks that they agree); value / terms, gradient max and gradient L2
   separately.  The whole-op inputs run every layer in the 32-row shape; the 128-row shape is covered per layer
   (tests/test_gpu_lpips_conv_layer_bf16x3.py).
2. It is closer to the exact float64 term than the bf16-operand arithmetic can be: the kernel's distance is below the float64
   bf16-operand form's.
3. Structure as for the float32 op: determinism, every element written, shapes, the region form, the capacity, capture.
4. ``MossStep`` with a bf16x3 net.

Every reference is computed on the CPU at test time or comes from the fixture.  Each test prints the figures it met."""
import ctypes

import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_gpu_lpips import K, _ratios, _run
from tests.test_gpu_lpips_bf16 import _net, _run_roi
from tests.test_gpu_moss_step import LRS, _fresh, _load, _release_device_memory, world  # noqa: F401  (fixtures of that module, by import)
from tests.test_lpips_bf16_cpu import CAPACITY_INPUT, MEASURES, bf16_reference, errors, images
from tests.test_lpips_bf16x3_cpu import GPU_INPUTS, exact_reference, split_record
from tests.test_lpips_cpu import load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net(gpu, hip_lib):
    return _net(gpu, "bf16x3")


@pytest.fixture(scope="module")
def net32(gpu, hip_lib):
    return _net(gpu, "f32")


@pytest.fixture(scope="module")
def net16(gpu, hip_lib):
    return _net(gpu, "bf16")


def test_the_net_holds_split_weights(gpu, net, net32, net16):
    """conv 1_1 float32; the twelve wide layers two bf16 planes in both layouts: hi the bf16 net's array bit for bit, lo the remainder
    of the float32 packing rounded to nearest even."""
    assert net.precision == "bf16x3" and net.w_fwd[0].dtype == torch.float32 and net.w_bwd[0].dtype == torch.float32
    assert torch.equal(net.w_fwd[0], net32.w_fwd[0]) and torch.equal(net.w_bwd[0], net32.w_bwd[0])
    for i in range(1, 13):
        for got, w16, w32 in ((net.w_fwd[i], net16.w_fwd[i], net32.w_fwd[i]), (net.w_bwd[i], net16.w_bwd[i], net32.w_bwd[i])):
            n = w32.numel()
            assert got.dtype == torch.bfloat16 and got.numel() == 2 * n
            assert torch.equal(got[:n], w16), i
            assert torch.equal(got[n:], (w32 - got[:n].float()).bfloat16()), i
            assert bool(got[n:].any())
    before = [w.clone() for w in net.w_fwd + net.w_bwd]
    net.refresh()
    assert net.precision == "bf16x3" and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(before, net.w_fwd + net.w_bwd))


# ---- 1. the kernel computes what it claims --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GPU_INPUTS)
def test_matches_the_split_form_in_float64(gpu, net, name):
    x, y = images(name)
    rec = split_record(name)
    value, terms, grad = _run(net, x.to(gpu), y.to(gpu))
    r = _ratios(value, terms, grad, rec)
    print(f"lpips bf16x3 {name}: total {rec['total']:.6g}, err32 {rec['value_err32']:.3g} / {rec['grad_err32_max']:.3g} / "
          f"{rec['grad_err32_l2']:.3g}, error / err32 = {r}")
    assert max(r.values()) <= K, r


def test_a_crop_below_its_capacity_meets_the_same_bar(gpu, net):
    """A 29 x 37 crop at (13,21) of a 64 x 64 frame under a 48 x 48 capacity, against the split form in float64 on the crop."""
    from moss_amd.loss import ViewRegion
    name, (h, w, x0, y0) = CAPACITY_INPUT, (29, 37, 13, 21)
    x, y = images(name)
    gen = torch.Generator().manual_seed(4)
    image, gt = torch.rand(3, 64, 64, generator=gen), torch.rand(3, 64, 64, generator=gen)
    image[:, y0:y0 + h, x0:x0 + w], gt[:, y0:y0 + h, x0:x0 + w] = x, y
    region = ViewRegion(torch.ones(1, 64, 64, device=gpu), rect=(x0, y0, w, h))
    value, terms, grad = _run_roi(net, image.to(gpu), gt.to(gpu), region, capacity=(48, 48))
    off = grad.clone()
    off[:, y0:y0 + h, x0:x0 + w] = 0
    assert not off.any()
    r = _ratios(value, terms, grad[:, y0:y0 + h, x0:x0 + w], split_record(name))
    print(f"lpips bf16x3 29x37 under a 48x48 capacity: error / err32 = {r}")
    assert max(r.values()) <= K, r


# ---- 2. closer to the truth than bf16 operands can be ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GPU_INPUTS)
def test_closer_to_float64_than_the_bf16_form(gpu, net, name):
    """Against the exact float64 term: on ``odd`` the kernel's value and gradient-L2 distances are below the float64 bf16-operand
    form's; on the person crop (where float32 itself is 4 % from float64 in the gradient) the value distance is.  The rest is printed."""
    x, y = images(name)
    exact = exact_reference(name)
    form = errors(bf16_reference(name), exact)
    value, terms, grad = _run(net, x.to(gpu), y.to(gpu))
    got = errors((terms.cpu(), value.cpu().reshape(()), grad.cpu()), exact)
    print(f"lpips bf16x3 {name}: distance from float64, kernel / bf16 form: " + ", ".join(f"{m} {got[m]:.3g} / {form[m]:.3g}" for m in MEASURES))
    assert got["value"] < form["value"]
    if name == "odd":
        assert got["grad_l2"] < form["grad_l2"]


def test_same_image_is_exactly_zero(gpu, net):
    x, y, _ = load_case("same", dtype=torch.float32, device=gpu)
    value, terms, grad = _run(net, x, y)
    assert float(value) == 0.0 and not terms.any() and not grad.any()


def test_the_three_precisions_differ(gpu, net, net32, net16):
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    a, b, c = _run(net, x, y), _run(net32, x, y), _run(net16, x, y)
    for other in (b, c):
        assert not torch.equal(a[0], other[0]) and not torch.equal(a[2], other[2])
    assert abs(float(a[0]) - float(b[0])) < 0.1 * float(b[0])


# ---- 3. structure ---------------------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_identical(gpu, net):
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    a, b = _run(net, x, y), _run(net, x, y)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_shapes_and_the_forward_that_keeps_nothing(gpu, net):
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


def test_every_gradient_element_is_written(gpu, net, hip_lib):
    """The split C entry points on a NaN-filled dL_dx, workspace and saved block: finite everywhere and equal to the autograd path's;
    a short workspace is refused under the new names with the float32 pair's text."""
    from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs, call
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)
    H, W = x.shape[1:]
    nan_bytes = lambda n: torch.full(((n + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    nws, nsv = hip_lib.moss_lpips_vgg_workspace_bytes(H, W), hip_lib.moss_lpips_vgg_saved_bytes(H, W)
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
    call("moss_lpips_vgg_forward_bf16x3", gpu, ctypes.byref(a))
    ws.fill_(float("nan"))
    b = LpipsVggBackwardArgs()
    b.H, b.W = H, W
    for i in range(13):
        b.weights_bwd[i] = net.w_bwd[i].data_ptr()
    b.scale, b.saved, b.g_out, b.dL_dx = net.scale.data_ptr(), saved.data_ptr(), g.data_ptr(), d_x.data_ptr()
    b.workspace, b.workspace_bytes = ws.data_ptr(), nws
    call("moss_lpips_vgg_backward_bf16x3", gpu, ctypes.byref(b))
    assert bool(torch.isfinite(d_x).all()) and bool(torch.isfinite(out).all())
    value, terms, grad = _run(net, x, y)
    assert torch.equal(d_x, grad) and torch.equal(out[:1], value.reshape(1)) and torch.equal(out[1:], terms)
    a.workspace_bytes = b.workspace_bytes = nws - 1
    with pytest.raises(RuntimeError, match="moss_lpips_vgg_forward_bf16x3.*workspace"):
        call("moss_lpips_vgg_forward_bf16x3", gpu, ctypes.byref(a))
    with pytest.raises(RuntimeError, match="moss_lpips_vgg_backward_bf16x3.*workspace"):
        call("moss_lpips_vgg_backward_bf16x3", gpu, ctypes.byref(b))
    with pytest.raises(RuntimeError, match="null pointer"):
        call("moss_lpips_vgg_pack_weights_bf16x3", gpu, 64, 64, None, None, None)


def test_region_form_and_capacity_equal_to_the_crop(gpu, net):
    """lpips_vgg_roi_fused on a 64 x 64 frame with a 37 x 29 rectangle at (13,21): equal to the op on the two crops bit for bit, zero
    off the rectangle; with ``capacity=`` the crop's size, bit-identical to the static call."""
    from moss_amd.loss import ViewRegion
    gen = torch.Generator().manual_seed(3)
    image, gt = torch.rand(3, 64, 64, generator=gen).to(gpu), torch.rand(3, 64, 64, generator=gen).to(gpu)
    x0, y0, w, h = 13, 21, 37, 29
    region = ViewRegion(torch.ones(1, 64, 64, device=gpu), rect=(x0, y0, w, h))
    value, terms, grad = _run_roi(net, image, gt, region)
    cv, ct, cg = _run(net, image[:, y0:y0 + h, x0:x0 + w], gt[:, y0:y0 + h, x0:x0 + w])
    assert torch.equal(value, cv) and torch.equal(terms, ct)
    assert torch.equal(grad[:, y0:y0 + h, x0:x0 + w], cg) and bool(cg.any())
    off = grad.clone()
    off[:, y0:y0 + h, x0:x0 + w] = 0
    assert not off.any()
    for u, v in zip(_run_roi(net, image, gt, region, capacity=(h, w)), (value, terms, grad)):
        assert torch.equal(u, v)


def test_capture_and_replay_with_new_inputs(gpu, net):
    """Forward + backward captured once, replayed over three input pairs: bit-identical to the eager op on those inputs."""
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


# ---- 4. MossStep ----------------------------------------------------------------------------------------------------------------------

def test_moss_step_with_a_bf16x3_net(gpu, hip_lib, world):
    """tests/test_gpu_moss_step.py's world with a bf16x3 LPIPS net: three replays of one capture equal three eager steps bit for bit."""
    from moss_amd.train import MossStep
    lp = mlp.cast_params(mlp.synthetic_weights(), device=gpu)
    lnet = mlp.LpipsVGG.from_tensors(lp["conv_weights"], lp["conv_biases"], lp["lin_weights"], lp["shift"], lp["scale"], precision="bf16x3")

    def step():
        pc, cam, _ = _fresh(world)
        return MossStep(pc, cam, world["gt"], world["bkgd"], world["region"], world["bg"], lnet, LRS), cam

    (eager, ce), (graphed, cg) = step(), step()
    graphed.capture(warmup=3)
    for k in range(3):
        _load(ce, k, gpu)
        _load(cg, k, gpu)
        out_e = eager.compute()
        te, ie = out_e["terms"].clone(), out_e["render"].clone()
        out_g = graphed()
        tg, ig = out_g["terms"].clone(), out_g["render"].clone()
        torch.cuda.synchronize(gpu)
        assert torch.equal(te, tg), (k, te.tolist(), tg.tolist())
        assert torch.equal(ie, ig), k
    graphed.check()
    assert graphed.dropped_frames == 0 and eager.step_counts() == graphed.step_counts() == (3, 3, 3)
    for a, b in zip(eager.optimizers, graphed.optimizers):
        assert torch.equal(a.flat_params, b.flat_params)
