"""The fused LPIPS term against a REFERENCE -- the ground truth's tapped activations computed once (``lpips_vgg_reference`` /
``lpips_vgg_roi_reference``; C ABI ``moss_lpips_vgg_reference`` / ``moss_lpips_vgg_forward_ref``) -- on the device.

The claim under test is "the same result with half the forward": bit for bit the two-image call where every wide convolution gets
the same kernel shape at M = H W as at M = 2 H W (a device with more than 122 CUs and a crop or capacity of up to 101 x 77: all layers
narrow either way), and within the bars of the two-image tests against float64 where the shapes differ (128 x 128 on 256 CUs: conv
1_2 is wide for two images and narrow for one).  The bars are those of tests/test_gpu_lpips.py (K = 8 x the float32 torch form's own
error), tests/test_gpu_lpips_bf16.py and tests/test_gpu_lpips_bf16x3.py; nothing here is tuned to the kernels.  The sizes are the
smallest at which each path can go wrong (tests/test_gpu_lpips_dynamic.py's regions, and one rectangle that overhangs the frame)."""
import ctypes

import pytest
import torch

from moss_amd import lpips as mlp
from tests.test_gpu_lpips import K, _ratios, _run
from tests.test_gpu_lpips_bf16 import _net, _run_roi
from tests.test_gpu_lpips_dynamic import CAP, FRAME, SIZES, _frames, _region
from tests.test_lpips_cpu import CASES, load_case, run_torch, weights

pytestmark = pytest.mark.gpu

PRECISIONS = mlp.ALL_PRECISIONS
OVERHANG = (37, 29, 40, 30)                                              # (h, w, x0, y0): past the right and bottom edges, so the origin is clamped
REGIONS = SIZES + [OVERHANG]


@pytest.fixture(scope="module")
def nets(gpu, hip_lib):
    return {p: _net(gpu, p) for p in PRECISIONS}


def _same_shapes_or_skip(gpu):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus <= 122:
        pytest.skip(f"{cus} CUs: a crop of up to 101 x 77 takes the narrow kernel shape with one image and with two only on a device "
                    "with more than 122 CUs; elsewhere the two calls agree to summation order, not bit for bit")


def _pair(gpu, case):
    if case == "rand101x77":
        gen = torch.Generator().manual_seed(101)
        return torch.rand(3, 101, 77, generator=gen).to(gpu), torch.rand(3, 101, 77, generator=gen).to(gpu)
    x, y, _ = load_case(case, dtype=torch.float32, device=gpu)
    return x, y


def _equal(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


# ---- 1. bit-identity, static ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["min", "odd", "strip", "rand101x77"])
def test_equals_the_two_image_call_bit_for_bit(gpu, nets, case, precision):
    _same_shapes_or_skip(gpu)
    net = nets[precision]
    x, y = _pair(gpu, case)
    ref = mlp.lpips_vgg_reference(net, y)
    assert ref.crop == tuple(x.shape[1:]) and ref.capacity is None and ref.precision == precision
    assert ref.nbytes == mlp.reference_bytes(*x.shape[1:]) and ref.generation == net.generation
    two = _run(net, x, y)
    assert float(two[0]) > 0 and bool(two[2].any())
    _equal(_run(net, x, ref), two)
    with torch.no_grad():
        vn, tn = mlp.lpips_vgg_fused(net, x.clone().requires_grad_(True), ref, return_terms=True)
    assert not vn.requires_grad
    _equal((vn, tn), two[:2])
    _equal((mlp.lpips_vgg_fused(net, x, ref),), two[:1])                # (an x that needs no gradient: nothing is kept)


# ---- 2. against float64 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_matches_reference_float64(gpu, nets, case):
    """Each fixture case through the reference path against the reference's float64 run, within K x its own float32 error; ``same``
    is exactly zero in value, terms and gradient."""
    net = nets["f32"]
    x, y, rec = load_case(case, dtype=torch.float32, device=gpu)
    value, terms, grad = _run(net, x, mlp.lpips_vgg_reference(net, y))
    assert value.shape == (1, 1, 1, 1) and grad.shape == x.shape
    if case == "same":
        assert float(value) == 0.0 and not terms.any() and not grad.any()
        return
    r = _ratios(value, terms, grad, rec)
    print(f"lpips reference {case}: error / err32 = {r}")
    assert max(r.values()) <= K, r


# ---- 3. where the shapes differ --------------------------------------------------------------------------------------------------------

def _record(precision, name):
    """The float64 statement of ``precision``'s arithmetic on the named input and the err32 of its float32 torch runs."""
    if precision == "bf16":
        from tests.test_lpips_bf16_cpu import bf16_record
        return bf16_record(name)
    if precision == "bf16x3":
        from tests.test_lpips_bf16x3_cpu import split_record
        return split_record(name)
    from tests.test_lpips_bf16_cpu import images
    x, y = images(name)
    t64, v64, g64 = run_torch(mlp.cast_params(weights(), torch.float64), x.double(), y.double())
    runs = [run_torch(weights(), x, y), run_torch(weights(), x, y, channels_last=True)]   # (as test_person_crop_against_the_torch_form)
    return {"terms": t64.numpy(), "total": float(v64), "grad": g64.numpy(),
            "value_err32": max(max(float((t.double() - t64).abs().max()), abs(float(v) - float(v64))) for t, v, _ in runs),
            "grad_err32_max": max(float((g.double() - g64).abs().max()) for _, _, g in runs),
            "grad_err32_l2": max(float((g.double() - g64).norm()) for _, _, g in runs)}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_where_the_kernel_shapes_differ(gpu, nets, precision):
    """A seeded 128 x 128 pair: on 256 CUs conv 1_2 has 2 * 16384 / 128 = 256 workgroups of the 128-row shape for two images and half
    of that for one, which then takes the 32-row shape: the two calls are not bit-compared.  The call against a reference meets the
    two-image call's own bar against the float64 torch form of its precision on the CPU.

    The pair is the person-like crop of tests/test_gpu_lpips.py (seed 7), as in every test of this suite whose kernel shapes differ
    from the yardstick's summation order (tests/test_gpu_lpips_dynamic.py::test_the_wide_kernel_shape_with_a_dynamic_size): err32 can
    carry the bar only if it contains what ANY float32 summation order does to this input, ReLU decisions at rounding distance from
    zero included, and on the near-black ground of a person crop the float32 torch runs have them.  Uniform noise does not qualify:
    at 128 x 128 (seed 11) its two float32 torch runs flip no ReLU, so err32 is summation noise alone (1.4e-12 on a gradient of 1.5e-6),
    while its float64 pre-activations come within 6e-7 of zero at typical size 1.7 -- the two GPU calls' ``saved`` blocks differ in
    exactly two sign bits of four million there (conv 2_2 and conv 3_3; winners and everything else equal), which alone is 5 000 x
    that err32.  Measured once, not part of the test."""
    from tests.test_lpips_bf16_cpu import images
    name = "person128x128"
    x, y = images(name)
    rec = _record(precision, name)
    assert rec["total"] > 1e-6 and rec["value_err32"] > 0 and rec["grad_err32_max"] > 0
    net = nets[precision]
    x, y = x.to(gpu), y.to(gpu)
    value, terms, grad = _run(net, x, mlp.lpips_vgg_reference(net, y))
    r = _ratios(value, terms, grad, rec)
    r2 = _ratios(*_run(net, x, y), rec)
    print(f"lpips reference {precision} 128x128 on {torch.cuda.get_device_properties(gpu).multi_processor_count} CUs: total "
          f"{rec['total']:.6g}, err32 {rec['value_err32']:.3g} / {rec['grad_err32_max']:.3g} / {rec['grad_err32_l2']:.3g}, "
          f"error / err32 against a reference = {r}, of the two-image call = {r2}")
    assert max(r.values()) <= K, r


# ---- 4. region and capacity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h, w, x0, y0, larger", [s + (False,) for s in REGIONS] + [s + (True,) for s in REGIONS if s[:2] != CAP])
def test_region_and_capacity(gpu, nets, h, w, x0, y0, larger, precision):
    """lpips_vgg_roi_reference then lpips_vgg_roi_fused against it, with the capacity equal to the crop and larger than it: value,
    terms and the full-frame gradient (zero off the crop) are the two-image region call's with that capacity."""
    _same_shapes_or_skip(gpu)
    net, cap = nets[precision], (CAP if larger else (h, w))
    image, gt = _frames(gpu, 3)
    region = _region(gpu, h, w, x0, y0)
    ref = mlp.lpips_vgg_roi_reference(net, gt, region, capacity=cap)
    assert ref.crop == (h, w) and ref.capacity == cap and ref.nbytes == mlp.reference_bytes(*cap)
    two = _run_roi(net, image, gt, region, cap)
    got = _run_roi(net, image, ref, region, cap)
    _equal(got, two)
    cx, cy = min(x0, FRAME[1] - w), min(y0, FRAME[0] - h)                # crop_origin
    off = got[2].clone()
    assert bool(off[:, cy:cy + h, cx:cx + w].any())
    off[:, cy:cy + h, cx:cx + w] = 0
    assert not off.any()


def test_static_region_call(gpu, nets):
    """Without a capacity: the reference of the region's crop, against the two-image region call."""
    _same_shapes_or_skip(gpu)
    net = nets["f32"]
    image, gt = _frames(gpu, 5)
    for size in (SIZES[0], OVERHANG):
        region = _region(gpu, *size)
        ref = mlp.lpips_vgg_roi_reference(net, gt, region)
        assert ref.capacity is None and ref.crop == size[:2]
        _equal(_run_roi(net, image, ref, region), _run_roi(net, image, gt, region))


# ---- 5. capture and replay -------------------------------------------------------------------------------------------------------------

def test_one_capture_three_views(gpu, nets):
    """Forward + backward against a STATIC reference captured once with capacity 64 x 48, replayed over three views of different crop
    sizes, each loaded by image.copy_, region.copy_ and ref_static.copy_(refs[k]): every replay is the eager two-image call on that
    view, bit for bit."""
    from moss_amd.graphs import capturing
    _same_shapes_or_skip(gpu)
    net = nets["f32"]
    sizes = SIZES[:2] + [OVERHANG]
    regions = [_region(gpu, *s) for s in sizes]
    frames = [_frames(gpu, 30 + k) for k in range(3)]
    refs, nbytes = mlp.reference_cache(net, [f[1] for f in frames], regions, CAP)
    assert nbytes == 3 * mlp.reference_bytes(*CAP) and [r.crop for r in refs] == [s[:2] for s in sizes]
    image = frames[0][0].clone()
    region = _region(gpu, *sizes[0])
    ref_static = mlp.LpipsReference.empty(net, CAP)
    assert ref_static.crop is None and ref_static.capacity == CAP and ref_static.nbytes == refs[0].nbytes
    with pytest.raises(ValueError, match="holds nothing yet"):
        mlp.lpips_vgg_roi_fused(net, image, ref_static, region, capacity=CAP)
    ref_static.copy_(refs[0])

    def fn():
        return _run_roi(net, image, ref_static, region, CAP)

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
    for k in (1, 2, 0):                                                  # (ends on the captured view, after two others)
        image.copy_(frames[k][0])
        region.copy_(regions[k])
        ref_static.copy_(refs[k])
        graph.replay()
        got = [v.clone() for v in outputs]
        torch.cuda.synchronize(gpu)
        assert ref_static.crop == sizes[k][:2]
        _equal(got, _run_roi(net, frames[k][0], frames[k][1], regions[k], CAP))
        seen.append(float(got[0]))
    assert len(set(seen)) == 3


# ---- 6. every element the consumer reads is written ------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("capacity", [None, CAP], ids=["static", "capacity"])
def test_nothing_depends_on_stale_buffers(gpu, nets, hip_lib, capacity, precision):
    """The C entry points on NaN-filled buffers: the reference block before the reference pass; ``saved``, the workspace and dL_dx
    before the forward against it and the backward.  With a capacity the block and ``saved`` are sized for it, so most of them lies
    beyond the 37 x 29 crop's rows and stays NaN.  Everything that comes out is finite and equal to the unpoisoned run."""
    from moss_amd._lib import LpipsVggBackwardArgs, LpipsVggForwardRefArgs, LpipsVggReferenceArgs, call
    net, suffix = nets[precision], mlp._SUFFIX[precision]
    h, w, x0, y0 = SIZES[0]
    image, gt = _frames(gpu, 3)
    region = _region(gpu, h, w, x0, y0)
    size = capacity or (h, w)
    nan_bytes = lambda n: torch.full(((n + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu)      # noqa: E731
    nws, nsv, nref = (getattr(hip_lib, f"moss_lpips_vgg_{k}_bytes")(*size) for k in ("workspace", "saved", "reference"))
    assert nws > 0 and nsv > 0 and nref == mlp.reference_bytes(*size) > 0
    ws, saved, block, d_x = nan_bytes(nws), nan_bytes(nsv), nan_bytes(nref), torch.full((3,) + FRAME, float("nan"), device=gpu)
    out, g = torch.full((6,), float("nan"), device=gpu), torch.ones(1, device=gpu)

    def common(blk):
        blk.rect = region.rect.data_ptr()
        blk.frame_H, blk.frame_W = FRAME
        if capacity:
            blk.cap_H, blk.cap_W = capacity                              # (H, W stay 0: ignored with a capacity)
        else:
            blk.H, blk.W = h, w
        blk.workspace, blk.workspace_bytes = ws.data_ptr(), nws

    r = LpipsVggReferenceArgs()
    common(r)
    r.y, r.reference, r.reference_bytes = gt.data_ptr(), block.data_ptr(), nref
    a = LpipsVggForwardRefArgs()
    common(a)
    a.x, a.reference, a.reference_bytes = image.data_ptr(), block.data_ptr(), nref
    for blk in (r, a):
        for i in range(13):
            blk.weights[i], blk.biases[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr()
        blk.shift, blk.scale = net.shift.data_ptr(), net.scale.data_ptr()
    for i in range(5):
        a.lin[i] = net.lin[i].data_ptr()
    a.out, a.terms, a.saved = out.data_ptr(), out[1:].data_ptr(), saved.data_ptr()
    call("moss_lpips_vgg_reference" + suffix, gpu, ctypes.byref(r))
    ws.fill_(float("nan"))
    call("moss_lpips_vgg_forward_ref" + suffix, gpu, ctypes.byref(a))
    ws.fill_(float("nan"))
    b = LpipsVggBackwardArgs()
    common(b)
    for i in range(13):
        b.weights_bwd[i] = net.w_bwd[i].data_ptr()
    b.scale, b.saved, b.g_out, b.dL_dx = net.scale.data_ptr(), saved.data_ptr(), g.data_ptr(), d_x.data_ptr()
    call("moss_lpips_vgg_backward" + suffix, gpu, ctypes.byref(b))
    assert bool(torch.isfinite(d_x).all()) and bool(torch.isfinite(out).all())
    ref = mlp.lpips_vgg_roi_reference(net, gt, region, capacity=capacity)
    rows = [(h >> l) * (w >> l) * c for l, c in enumerate(mlp.TAP_CHANNELS)]
    offs = [0]
    for l, c in enumerate(mlp.TAP_CHANNELS):
        offs.append(offs[-1] + ((size[0] >> l) * (size[1] >> l) * c * 4 + 255) // 256 * 256)
    assert offs[-1] == nref
    mine = ref.block.view(torch.float32)
    for l in range(5):                                                   # the rows the taps read: written, and the same both times
        lo = offs[l] // 4
        assert bool(torch.isfinite(block[lo:lo + rows[l]]).all()), l
        assert torch.equal(block[lo:lo + rows[l]], mine[lo:lo + rows[l]]), l
    if capacity:
        assert bool(torch.isnan(block).any())                            # (beyond the actual rows nothing was written, and nothing read)
    value, terms, grad = _run_roi(net, image, ref, region, capacity)
    assert torch.equal(d_x, grad) and torch.equal(out[:1], value.reshape(1)) and torch.equal(out[1:], terms)


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_determinism(gpu, nets, precision):
    net = nets[precision]
    x, y = _pair(gpu, "odd")
    a, b = mlp.lpips_vgg_reference(net, y), mlp.lpips_vgg_reference(net, y)
    assert a.block.data_ptr() != b.block.data_ptr() and torch.equal(a.block, b.block)
    _equal(_run(net, x, a), _run(net, x, a))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals(gpu, nets):
    net = nets["f32"]
    x, y = _pair(gpu, "odd")                                             # 37 x 53
    ref = mlp.lpips_vgg_reference(net, y)
    mlp.lpips_vgg_fused(net, x, ref)
    with pytest.raises(ValueError, match="precision='f32' net and this net has precision='bf16'"):
        mlp.lpips_vgg_fused(nets["bf16"], x, ref)
    with pytest.raises(ValueError, match="precision='bf16x3' net and this net has precision='f32'"):
        mlp.lpips_vgg_fused(net, x, mlp.lpips_vgg_reference(nets["bf16x3"], y))
    other = _net(gpu, "f32")
    stale = mlp.lpips_vgg_reference(other, y)
    with pytest.raises(ValueError, match="or by another net"):
        mlp.lpips_vgg_fused(net, x, stale)
    mlp.lpips_vgg_fused(other, x, stale)
    other.refresh()
    with pytest.raises(ValueError, match="before net.refresh"):
        mlp.lpips_vgg_fused(other, x, stale)
    _equal(_run(other, x, mlp.lpips_vgg_reference(other, y)), _run(net, x, ref))      # (made again: the same weights, the same bits)
    elsewhere = mlp.LpipsReference(ref.block.cpu(), ref.crop, None, "f32", net.generation)
    with pytest.raises(ValueError, match="the reference is on cpu"):
        mlp.lpips_vgg_fused(net, x, elsewhere)
    with pytest.raises(ValueError, match="holds a 37x53 crop and the call's is 37x52"):
        mlp.lpips_vgg_fused(net, x[:, :, :52], ref)
    image, gt = _frames(gpu, 3)
    region = _region(gpu, *SIZES[0])                                      # 37 x 29
    with_cap = mlp.lpips_vgg_roi_reference(net, gt, region, capacity=CAP)
    without = mlp.lpips_vgg_roi_reference(net, gt, region)
    for bad, cap in ((with_cap, None), (with_cap, (48, 48)), (without, CAP)):
        with pytest.raises(ValueError, match="laid out for capacity"):
            mlp.lpips_vgg_roi_fused(net, image, bad, region, capacity=cap)
    with pytest.raises(ValueError, match="laid out for capacity"):
        mlp.lpips_vgg_fused(net, image, with_cap)
    for good, cap in ((with_cap, CAP), (without, None)):
        with pytest.raises(ValueError, match="holds a 37x29 crop and the call's is 16x16"):
            mlp.lpips_vgg_roi_fused(net, image, good, _region(gpu, *SIZES[1]), capacity=cap)
    with pytest.raises(ValueError, match="laid out differently"):
        with_cap.copy_(without)
    made = mlp.lpips_vgg_reference(net, y.clone().requires_grad_(True))   # (no-grad semantics: nothing is recorded, nothing refused)
    assert not made.block.requires_grad and torch.equal(made.block, ref.block)
    with pytest.raises(ValueError, match=">= 16"):
        mlp.lpips_vgg_reference(net, y[:, :15])


def _views(gpu):
    """tests/test_gpu_lpips.py's evaluate_views set-up at 64 x 48."""
    from moss_amd import scenes
    from moss_amd.gaussian_model import GaussianSet
    from moss_amd.gaussian_renderer import camera_view
    from moss_amd.loss import ViewRegion
    H, W = 64, 48
    scene = scenes.config2()
    c0 = scene.camera
    s = W / c0.W
    cams = [camera_view(scenes.make_camera(W, H, float(c0.K[0, 0]) * s, float(c0.K[1, 1]) * s, W / 2, H / 2, R, t), gpu)
            for R, t in scenes.look_at_ring(3)]
    pc = GaussianSet(scene, sh_degree=3, device=gpu, unified_features=True)
    gen = torch.Generator().manual_seed(5)
    gts = [1.5 * torch.rand(3, H, W, generator=gen).to(gpu) - 0.25 for _ in range(3)]      # (beyond [0, 1]: the clamp matters)
    mask = torch.zeros(1, H, W, device=gpu)
    mask[:, 4:60, 3:43] = 1
    return pc, cams, gts, [ViewRegion(mask), None, ViewRegion(mask)], torch.zeros(3, device=gpu)


# ---- 9. evaluate_views -----------------------------------------------------------------------------------------------------------------

def test_evaluate_views_with_references(gpu, nets):
    """Three 64 x 48 views: with one reference per view, made from the clamped ground truth, all four means are those of
    evaluate_views(lpips=net); references of a bf16 net are refused before anything is rendered."""
    from moss_amd.metrics import evaluate_views
    _same_shapes_or_skip(gpu)
    net = nets["f32"]
    pc, cams, gts, regions, bg = _views(gpu)
    want = evaluate_views(pc, cams, gts, regions, bg, lpips=net)
    refs = [mlp.lpips_vgg_reference(net, torch.clamp(g, 0.0, 1.0)) for g in gts]
    got = evaluate_views(pc, cams, gts, regions, bg, lpips=net, lpips_references=refs)
    assert want["lpips"] > 0 and got == want, (got, want)
    unclamped = evaluate_views(pc, cams, gts, regions, bg, lpips=net, lpips_references=[mlp.lpips_vgg_reference(net, g) for g in gts])
    assert unclamped["lpips"] != want["lpips"]
    bf16 = [mlp.lpips_vgg_reference(nets["bf16"], torch.clamp(g, 0.0, 1.0)) for g in gts]
    with pytest.raises(ValueError, match="float32 term"):
        evaluate_views(pc, cams, gts, regions, bg, lpips=net, lpips_references=bf16)
    with pytest.raises(ValueError, match="one LPIPS reference per camera"):
        evaluate_views(pc, cams, gts, regions, bg, lpips=net, lpips_references=refs[:2])
