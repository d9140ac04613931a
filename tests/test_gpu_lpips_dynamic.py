"""The LPIPS call whose crop SIZE is read from the device (``lpips_vgg_roi_fused(capacity=)``; ``cap_H``, ``cap_W`` of the C ABI) on the
device: bit for bit the static op where the kernel shapes agree, independent of where the crop sits, within the project's bar of
float64 where the shapes differ, one capture replayed over crops of three sizes, the refusals, and ``MossStep(lpips_capacity=)``.

The shapes are the smallest at which each path can go wrong: every level odd (37 x 29 -> 18 x 14, 9 x 7, 4 x 3, 2 x 1), the minimum
(16 x 16: the last tap is 1 x 1), crop = capacity, one axis at capacity; 144 x 128 is the smallest capacity whose first wide layer
takes the 128-row kernel shape on a 256-CU device.  The bar of the float64 comparison is tests/test_gpu_lpips.py's (K = 8)."""
import ctypes

import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_gpu_lpips import K, _person_crop, _ratios
from tests.test_gpu_lpips import _run as _run_static
from tests.test_gpu_moss_step import LRS, _fresh, _load, _release_device_memory, world  # noqa: F401  (fixtures of that module, by import)
from tests.test_lpips_cpu import load_case, run_torch, weights

pytestmark = pytest.mark.gpu

FRAME = (64, 64)
CAP = (64, 48)                                                           # (cap_h, cap_w)
# (h, w, x0, y0): odd at every level; the minimum; crop = capacity; one axis at capacity and the other just above the minimum
SIZES = [(37, 29, 13, 21), (16, 16, 5, 7), (64, 48, 11, 0), (17, 48, 15, 3)]


@pytest.fixture(scope="module")
def net(gpu, hip_lib):
    p = mlp.cast_params(weights(), device=gpu)
    return mlp.LpipsVGG.from_tensors(p["conv_weights"], p["conv_biases"], p["lin_weights"], p["shift"], p["scale"])


def _region(gpu, h, w, x0, y0, frame=FRAME):
    from moss_amd.loss import ViewRegion
    return ViewRegion(torch.ones(1, *frame, device=gpu), rect=(x0, y0, w, h))


def _frames(gpu, seed, frame=FRAME):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(3, *frame, generator=gen).to(gpu), torch.rand(3, *frame, generator=gen).to(gpu)


def _run(net, image, gt, region, capacity):
    """(value, terms, dL/d image over the whole frame) of the region form, detached."""
    image = image.detach().requires_grad_(True)
    value, terms = mlp.lpips_vgg_roi_fused(net, image, gt, region, return_terms=True, capacity=capacity)
    (grad,) = torch.autograd.grad(value.sum(), image)
    return value.detach(), terms.detach(), grad.detach()


def _assert_equals_static(net, got, image, gt, h, w, x0, y0):
    """``got`` = (value, terms, frame gradient) against lpips_vgg_fused on the two crops, bit for bit; zero off the rectangle."""
    value, terms, grad = got
    cv, ct, cg = _run_static(net, image[:, y0:y0 + h, x0:x0 + w], gt[:, y0:y0 + h, x0:x0 + w])
    assert torch.equal(value, cv) and torch.equal(terms, ct)
    assert torch.equal(grad[:, y0:y0 + h, x0:x0 + w], cg) and bool(cg.any())
    off = grad.clone()
    off[:, y0:y0 + h, x0:x0 + w] = 0
    assert not off.any()


@pytest.mark.parametrize("h, w, x0, y0", SIZES)
def test_equals_the_static_op_bit_for_bit(gpu, net, h, w, x0, y0):
    """Under a 64 x 48 capacity every layer takes the narrow kernel shape, as the static op at any of these crops does: value, the five
    terms and the gradient inside the rectangle are the static op's on the two crops, and the gradient is zero off the rectangle."""
    image, gt = _frames(gpu, 3)
    _assert_equals_static(net, _run(net, image, gt, _region(gpu, h, w, x0, y0), CAP), image, gt, h, w, x0, y0)


def test_nothing_depends_on_stale_buffers(gpu, net, hip_lib):
    """The C entry points with a capacity on a NaN-filled dL_dx, workspace and saved block (both sized for the capacity, so most of
    them lies beyond the 37 x 29 crop's extents): everything comes back finite and equal to the autograd path's."""
    from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs, call
    h, w, x0, y0 = SIZES[0]
    image, gt = _frames(gpu, 3)
    region = _region(gpu, h, w, x0, y0)
    nan_bytes = lambda n: torch.full(((n + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    nws, nsv = hip_lib.moss_lpips_vgg_workspace_bytes(*CAP), hip_lib.moss_lpips_vgg_saved_bytes(*CAP)
    assert nws > hip_lib.moss_lpips_vgg_workspace_bytes(h, w) > 0 and nsv > hip_lib.moss_lpips_vgg_saved_bytes(h, w) > 0
    ws, saved, d_x = nan_bytes(nws), nan_bytes(nsv), torch.full((3,) + FRAME, float("nan"), device=gpu)
    out, g = torch.full((6,), float("nan"), device=gpu), torch.ones(1, device=gpu)
    a = LpipsVggArgs()
    a.x, a.y, a.rect = image.data_ptr(), gt.data_ptr(), region.rect.data_ptr()
    a.frame_H, a.frame_W = FRAME
    a.cap_H, a.cap_W = CAP                                               # (H, W stay 0: ignored with a capacity)
    for i in range(13):
        a.weights[i], a.biases[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr()
    for i in range(5):
        a.lin[i] = net.lin[i].data_ptr()
    a.shift, a.scale, a.out, a.terms = net.shift.data_ptr(), net.scale.data_ptr(), out.data_ptr(), out[1:].data_ptr()
    a.saved, a.workspace, a.workspace_bytes = saved.data_ptr(), ws.data_ptr(), nws
    call("moss_lpips_vgg_forward", gpu, ctypes.byref(a))
    ws.fill_(float("nan"))
    b = LpipsVggBackwardArgs()
    b.rect = region.rect.data_ptr()
    b.frame_H, b.frame_W = FRAME
    b.cap_H, b.cap_W = CAP
    for i in range(13):
        b.weights_bwd[i] = net.w_bwd[i].data_ptr()
    b.scale, b.saved, b.g_out, b.dL_dx = net.scale.data_ptr(), saved.data_ptr(), g.data_ptr(), d_x.data_ptr()
    b.workspace, b.workspace_bytes = ws.data_ptr(), nws
    call("moss_lpips_vgg_backward", gpu, ctypes.byref(b))
    assert bool(torch.isfinite(d_x).all()) and bool(torch.isfinite(out).all())
    value, terms, grad = _run(net, image, gt, region, CAP)
    assert torch.equal(d_x, grad) and torch.equal(out[:1], value.reshape(1)) and torch.equal(out[1:], terms)
    _assert_equals_static(net, (out[:1].reshape(1, 1, 1, 1), out[1:], d_x), image, gt, h, w, x0, y0)


def test_placement_does_not_matter(gpu, net):
    """One 37 x 29 crop's content in two frames that differ everywhere else: at an odd offset, and with a rectangle that overhangs
    the frame's bottom-right corner, which crop_origin moves back to fit.  The same value and terms; the same gradient, shifted."""
    h, w = 37, 29
    x, y, _ = load_case("odd", dtype=torch.float32, device=gpu)          # 37 x 53
    x, y = x[:, :, :w].contiguous(), y[:, :, :w].contiguous()
    results = []
    for seed, (x0, y0), corner in ((11, (13, 21), (13, 21)), (12, (40, 30), (FRAME[1] - w, FRAME[0] - h))):
        image, gt = _frames(gpu, seed)
        cx, cy = corner
        image[:, cy:cy + h, cx:cx + w] = x
        gt[:, cy:cy + h, cx:cx + w] = y
        value, terms, grad = _run(net, image, gt, _region(gpu, h, w, x0, y0), CAP)
        off = grad.clone()
        off[:, cy:cy + h, cx:cx + w] = 0
        assert not off.any()
        results.append((value, terms, grad[:, cy:cy + h, cx:cx + w].clone()))
    for u, v in zip(*results):
        assert torch.equal(u, v)
    cv, ct, cg = _run_static(net, x, y)
    assert torch.equal(results[0][0], cv) and torch.equal(results[0][1], ct) and torch.equal(results[0][2], cg)


def test_the_wide_kernel_shape_with_a_dynamic_size(gpu, net):
    """Capacity 144 x 128 on a 160 x 144 frame: conv 1_2 has 2 * 144 * 128 / 128 = 288 workgroups of the 128-row shape, at least the
    CU count, so that shape runs -- on a 101 x 77 crop, for which the static op takes the narrow shape: the two are not bit-compared.
    The reference is lpips_vgg_torch on the CPU crops: float64, and float32 twice for the three err32 numbers, as
    tests/test_gpu_lpips.py::test_person_crop_against_the_torch_form forms them; all three ratios within K = 8.  Twice: the same bits."""
    frame, cap, (h, w, x0, y0) = (160, 144), (144, 128), (101, 77, 31, 17)
    assert torch.cuda.get_device_properties(gpu).multi_processor_count <= 2 * cap[0] * cap[1] // 128
    x, y = _person_crop(h, w)
    t64, v64, g64 = run_torch(mlp.cast_params(weights(), torch.float64), x.double(), y.double())
    runs = [run_torch(weights(), x, y), run_torch(weights(), x, y, channels_last=True)]
    rec = {"terms": t64.numpy(), "total": float(v64), "grad": g64.numpy(),
           "value_err32": max(max(float((t.double() - t64).abs().max()), abs(float(v) - float(v64))) for t, v, _ in runs),
           "grad_err32_max": max(float((g.double() - g64).abs().max()) for _, _, g in runs),
           "grad_err32_l2": max(float((g.double() - g64).norm()) for _, _, g in runs)}
    assert float(v64) > 1e-6 and rec["value_err32"] > 0 and rec["grad_err32_max"] > 0
    image, gt = _frames(gpu, 21, frame)
    image[:, y0:y0 + h, x0:x0 + w] = x.to(gpu)
    gt[:, y0:y0 + h, x0:x0 + w] = y.to(gpu)
    region = _region(gpu, h, w, x0, y0, frame)
    value, terms, grad = _run(net, image, gt, region, cap)
    r = _ratios(value, terms, grad[:, y0:y0 + h, x0:x0 + w], rec)
    print(f"lpips dynamic {h}x{w} under {cap[0]}x{cap[1]}: total {float(v64):.6g}, err32 {rec['value_err32']:.3g} / "
          f"{rec['grad_err32_max']:.3g} / {rec['grad_err32_l2']:.3g}, error / err32 = {r}")
    assert max(r.values()) <= K, r
    off = grad.clone()
    off[:, y0:y0 + h, x0:x0 + w] = 0
    assert not off.any()
    for u, v in zip((value, terms, grad), _run(net, image, gt, region, cap)):
        assert torch.equal(u, v)


def test_one_capture_three_crop_sizes(gpu, net):
    """Forward + backward captured ONCE (a host synchronisation would fail the capture) with capacity 64 x 48, replayed on three
    frames whose regions -- 37 x 29, 16 x 16, 64 x 48 -- are swapped in by region.copy_: every replay is bit-identical to the eager
    static op on that frame's crops."""
    from moss_amd.graphs import capturing
    views = [(_region(gpu, *s), s, _frames(gpu, 30 + k)) for k, s in enumerate(SIZES[:3])]
    image, gt = (t.clone() for t in views[0][2])
    region = _region(gpu, *SIZES[0])

    def fn():
        return _run(net, image, gt, region, CAP)

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
    for other, (h, w, x0, y0), (fx, fy) in views[1:] + views[:1]:       # (ends on the captured size, after two others)
        image.copy_(fx)
        gt.copy_(fy)
        region.copy_(other)
        graph.replay()
        got = [v.clone() for v in outputs]
        torch.cuda.synchronize(gpu)
        _assert_equals_static(net, got, fx, fy, h, w, x0, y0)
        seen.append(float(got[0]))
    assert len(set(seen)) == 3


def _blocks(net, gpu, hip_lib, image, gt, region):
    """Valid forward and backward argument blocks with capacity CAP on the 64 x 64 frame (buffers kept alive by the caller)."""
    from moss_amd._lib import LpipsVggArgs, LpipsVggBackwardArgs
    nws, nsv = hip_lib.moss_lpips_vgg_workspace_bytes(*CAP), hip_lib.moss_lpips_vgg_saved_bytes(*CAP)
    keep = {"ws": torch.empty(nws, dtype=torch.uint8, device=gpu), "saved": torch.empty(nsv, dtype=torch.uint8, device=gpu),
            "out": torch.zeros(6, device=gpu), "g": torch.ones(1, device=gpu), "d_x": torch.zeros((3,) + FRAME, device=gpu)}
    a, b = LpipsVggArgs(), LpipsVggBackwardArgs()
    a.x, a.y = image.data_ptr(), gt.data_ptr()
    for blk in (a, b):
        blk.rect = region.rect.data_ptr()
        blk.frame_H, blk.frame_W = FRAME
        blk.cap_H, blk.cap_W = CAP
        blk.workspace, blk.workspace_bytes = keep["ws"].data_ptr(), nws
        blk.saved = keep["saved"].data_ptr()
    for i in range(13):
        a.weights[i], a.biases[i], b.weights_bwd[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr(), net.w_bwd[i].data_ptr()
    for i in range(5):
        a.lin[i] = net.lin[i].data_ptr()
    a.shift, a.scale, a.out, a.terms = net.shift.data_ptr(), net.scale.data_ptr(), keep["out"].data_ptr(), keep["out"][1:].data_ptr()
    b.scale, b.g_out, b.dL_dx = net.scale.data_ptr(), keep["g"].data_ptr(), keep["d_x"].data_ptr()
    return a, b, keep


def test_refusals(gpu, net, hip_lib):
    """Through the C ABI, forward and backward alike: a capacity with rect NULL, outside the range, larger than the frame, only one
    of cap_H / cap_W, a short workspace; through Python: a region that exceeds the capacity."""
    from moss_amd._lib import call
    image, gt = _frames(gpu, 3)
    region = _region(gpu, *SIZES[0])
    a, b, keep = _blocks(net, gpu, hip_lib, image, gt, region)
    for name, blk in (("moss_lpips_vgg_forward", a), ("moss_lpips_vgg_backward", b)):
        call(name, gpu, ctypes.byref(blk))                               # the blocks are good as they stand
        for field, value, why in (("rect", None, "needs rect"), ("cap_H", 15, "capacity must be >= 16"),
                                  ("cap_W", 1 << 20, "capacity must be >= 16"), ("cap_H", 65, "larger than the frame"),
                                  ("cap_W", 65, "larger than the frame"), ("cap_H", 0, "both be set"), ("cap_W", 0, "both be set"),
                                  ("workspace_bytes", blk.workspace_bytes - 1, "workspace"), ("workspace", None, "workspace")):
            old = getattr(blk, field)
            setattr(blk, field, value)
            with pytest.raises(RuntimeError, match=why):
                call(name, gpu, ctypes.byref(blk))
            setattr(blk, field, old)
        call(name, gpu, ctypes.byref(blk))
    # a workspace that would do for the crop but not for the capacity
    a.workspace_bytes = hip_lib.moss_lpips_vgg_workspace_bytes(SIZES[0][0], SIZES[0][1])
    with pytest.raises(RuntimeError, match="workspace"):
        call("moss_lpips_vgg_forward", gpu, ctypes.byref(a))
    torch.cuda.synchronize(gpu)
    with pytest.raises(ValueError, match="exceeds the capacity"):
        mlp.lpips_vgg_roi_fused(net, image, gt, region, capacity=(36, 48))
    with pytest.raises(ValueError, match="exceeds the capacity"):
        mlp.lpips_vgg_roi_fused(net, image, gt, region, capacity=(48, 28))
    with pytest.raises(ValueError, match="capacity must be"):
        mlp.lpips_vgg_roi_fused(net, image, gt, region, capacity=(65, 48))


# ---- MossStep ------------------------------------------------------------------------------------------------------------------------

def _moss_regions(world, gpu):
    """Three regions of different sizes on the 512 x 512 frame; the first is tests/test_gpu_moss_step.py's (192 wide, 256 high)."""
    from moss_amd.loss import ViewRegion
    out = []
    for x0, y0, w, h in ((160, 128, 192, 256), (171, 101, 150, 301), (133, 157, 233, 177)):
        bound = torch.zeros(1, world["H"], world["W"])
        bound[:, y0:y0 + h, x0:x0 + w] = 1
        out.append(ViewRegion(bound.to(gpu)))
    assert [r.xywh for r in out] == [(160, 128, 192, 256), (171, 101, 150, 301), (133, 157, 233, 177)]
    return out


def _moss_step(world, gpu, capacity):
    from moss_amd.train import MossStep
    pc, cam, _ = _fresh(world)
    region = _moss_regions(world, gpu)[0]                                # (a region of the step's own: a static input it rewrites)
    assert region.xywh == world["region"].xywh and torch.equal(region.rect, world["region"].rect)
    return MossStep(pc, cam, world["gt"], world["bkgd"], region, world["bg"], world["lpips"], LRS, lpips_capacity=capacity), cam


def test_moss_step_replays_frames_whose_crops_differ(gpu, hip_lib, world):
    """One capture with lpips_capacity = the frame, replayed over three frames whose regions differ in size, against the eager
    compute() of a second identically-initialised step fed the same frames: the same bits in ``terms`` and in the render."""
    regions = _moss_regions(world, gpu)
    (eager, ce), (graphed, cg) = _moss_step(world, gpu, "frame"), _moss_step(world, gpu, "frame")
    assert graphed.lpips_capacity == (world["H"], world["W"])
    graphed.capture(warmup=3)
    lpips_terms = []
    for i in (1, 2, 0, 1):
        for step, cam in ((eager, ce), (graphed, cg)):
            _load(cam, i, gpu)
            step.region.copy_(regions[i])
        out_e = eager.compute()
        te, ie = out_e["terms"].clone(), out_e["render"].clone()
        out_g = graphed()
        tg, ig = out_g["terms"].clone(), out_g["render"].clone()
        torch.cuda.synchronize(gpu)
        assert torch.equal(te, tg), (i, te.tolist(), tg.tolist())
        assert torch.equal(ie, ig), i
        lpips_terms.append(float(tg[3]))
    assert len(set(lpips_terms)) == 4 and all(v > 0 for v in lpips_terms)
    graphed.check()                                                      # (the regions fit the capacity: nothing to refuse)
    assert graphed.dropped_frames == 0
    eager.context.check_status()
    assert eager.step_counts() == graphed.step_counts() == (4, 4, 4)


def test_moss_step_without_a_capacity_refuses_another_crop_size(gpu, hip_lib, world):
    """Without lpips_capacity the crop's size is in the captured LPIPS launches: check() passes while the region keeps its size and
    raises once a region of another size has been swapped in."""
    regions = _moss_regions(world, gpu)
    step, cam = _moss_step(world, gpu, None)
    step.capture(warmup=2)
    step()
    step.check()
    step.region.copy_(regions[1])
    step()
    torch.cuda.synchronize(gpu)
    with pytest.raises(RuntimeError, match="LPIPS was captured at 256x192"):
        step.check()
