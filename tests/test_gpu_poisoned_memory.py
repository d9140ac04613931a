"""Every op on poisoned allocator memory: nothing is read before it is written.

Almost every op here takes its outputs and scratch from ``torch.empty`` on the promise that the kernels write every element first.
Early in a process the caching allocator hands out fresh, zeroed pages -- the one content that hides a missing write -- while a long
training run gets recycled memory on every step.  Each case below runs an op with ``tests.helpers.poisoned_allocator`` under the fills

    0x00  the benign case (twice: run-to-run determinism comes first; every op here is bit-reproducible),
    0xFF  float NaN, int -1, bool true,
    0x3C  float ~0.0115, a large positive int: a finite value gets through ``x > 0 ? x : 0`` guards that swallow NaN,

and requires its documented results -- returned values and gradients; of a list with a count its first ``count`` entries -- to be
BIT-identical across them (floats are compared through their integer views, so -0 and +0 differ and equal NaNs do not).  The opaque
contents of saved / geom / binning / img buffers and workspaces are not compared; what is computed from them is (a backward on a
poisoned forward's buffers).  Whether the clean result is RIGHT is the other modules' business.  Inputs are made before the seeding and
lie outside the poison; in every case the helper's three self-checks hold: the canaries came back poisoned, no fresh segment came from
the driver inside the block, and the tensors the op returned lie inside the seeded ranges.  Only eager calls: captured graphs allocate
from private pools.  Shapes are the smallest with the risky structure."""
import gc
import os

import numpy as np
import pytest
import torch

from moss_amd import scenes
from tests import helpers as hp
from tests.test_gpu_ops import _raw_params, _stacked_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _bits(t):
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))
    return type(a) is type(b) and a == b


def _plus_zero(t):
    """Every element is +0: not a tiny number, not -0."""
    return not bool(_bits(t.contiguous()).any())


def under_fills(gpu, prepare, run):
    """``prepare()`` makes the op's inputs (before the seeding); ``run(inputs)`` calls the op and returns ``(results, also_owned)``: a dict
    of documented results (tensors, ints; None entries are dropped) and further tensors the op allocated.  Every tensor of both must lie
    in poisoned memory.  Returns the (CPU) results of the first 0x00 run after requiring the other three to equal them bit for bit."""
    runs = []
    fills = (0x00,) + hp.POISON_FILLS
    for byte in fills:
        gc.collect()
        inputs = prepare()
        with hp.poisoned_allocator(gpu, byte) as poison:
            res, also = run(inputs)
            res = {k: v for k, v in res.items() if v is not None}
            poison.assert_owns(*[v for v in res.values() if isinstance(v, torch.Tensor) and v.is_cuda], *also)
            torch.cuda.synchronize(gpu)
            res = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
            del also
        del inputs
        runs.append(res)
    for i, (byte, r) in enumerate(zip(fills, runs)):
        assert r.keys() == runs[0].keys()
        for k in r:
            assert _same(runs[0][k], r[k]), (f"{k}: two runs on zero-filled memory differ (not deterministic)" if i == 1 else
                                             f"{k} differs when the allocator's memory is filled with 0x{byte:02X}")
    return runs[0]


def test_a_missing_write_is_caught(gpu, hip_lib):
    """The harness on an "op" with the bug it is here for: one element of a ``torch.empty`` result is never written.  Both zero-filled
    runs agree (that is how the bug hides); the 0xFF run must be reported.  An op that writes everything passes."""
    def leaky(a, skip):
        out = torch.empty(3 * 4097, device=gpu)                          # small pool ...
        big = torch.empty(3 << 20, device=gpu)                           # ... and large pool
        out[:skip].copy_(a["x"][:skip]); out[skip + 1:].copy_(a["x"][skip + 1:])
        big.fill_(1.5)
        return {"out": out, "big": big}, []

    prepare = lambda: dict(x=torch.arange(3 * 4097, dtype=torch.float32).to(gpu))      # noqa: E731
    with pytest.raises(AssertionError, match="out differs when the allocator's memory is filled with 0xFF"):
        under_fills(gpu, prepare, lambda a: leaky(a, 4096))
    under_fills(gpu, prepare, lambda a: leaky(a, 3 * 4097))              # (skip = the length: nothing is left out)


# ---------------------------------------------------------------- rasterizer
def _scene_a():
    """config1 on a 70 x 50 image (ragged against the 16 x 16 tiles), P = 250 (no multiple of 64), every third Gaussian behind the camera."""
    s = scenes.config1(P=250, W=70, H=50)
    s.means3D[::3, 2] -= 10.0
    s.cov3D_precomp = scenes.covariance_precomp(s.scales, s.rotations, 1.0, s.transforms)
    return s


def _raster_inputs(d, gpu, raw=False, depth_grad=True):
    c = d.cam
    dev = lambda t: torch.Tensor([]) if t is None else t.to(gpu)         # noqa: E731
    a = dict(bg=d.bg.to(gpu), means3D=d.means3D.to(gpu), colors=dev(d.colors_precomp), opacity=d.opacities.to(gpu), scales=dev(d.scales),
             rotations=dev(d.rotations), cov3D=dev(d.cov3D_precomp), view=c.viewmatrix.to(gpu), proj=c.projmatrix.to(gpu), sh=dev(d.shs),
             campos=c.campos.to(gpu), transforms=None if d.transforms is None else d.transforms.to(gpu))
    if raw:                                                               # the raw parameters whose getters give the scene's values
        g = torch.Generator().manual_seed(3)
        a["opacity"] = torch.logit(d.opacities).to(gpu)
        a["scales"] = torch.log(d.scales).to(gpu)
        a["rotations"] = (d.rotations * (0.2 + 3.0 * torch.rand(d.P, 1, generator=g))).to(gpu)
    dc, dd, da = hp.image_grads(d.H, d.W)
    a["dc"], a["dd"], a["da"] = dc.to(gpu), (dd.to(gpu) if depth_grad else None), da.to(gpu)
    return a


def _raster_run(d, a, tag="", raw_flags=0, all_outputs=False, context=None):
    """Forward, then the backward on that forward's buffers.  Returns (results, the three opaque buffers)."""
    from moss_amd.diff_gaussian_rasterization import _C
    c = d.cam
    kw = {} if a["transforms"] is None else {"transforms": a["transforms"]}
    if raw_flags:
        kw["raw_flags"] = raw_flags
    if context is not None:
        kw["context"] = context
    R, color, depth, alpha, radii, geom, binning, img = _C.rasterize_gaussians(
        a["bg"], a["means3D"], a["colors"], a["opacity"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"], a["view"], a["proj"],
        c.tanfovx, c.tanfovy, c.H, c.W, a["sh"], d.degree, a["campos"], False, False, **kw)
    if raw_flags:
        kw["opacities"] = a["opacity"]
    grads = _C.rasterize_gaussians_backward(
        a["bg"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], d.scale_modifier, a["cov3D"], a["view"], a["proj"],
        c.tanfovx, c.tanfovy, a["dc"], a["dd"], a["da"], a["sh"], d.degree, a["campos"], geom, R, binning, img, alpha, False,
        all_outputs=all_outputs, **kw)
    res = {tag + "color": color, tag + "depth": depth, tag + "alpha": alpha, tag + "radii": radii}
    if context is None:
        res[tag + "R"] = int(R)
    res.update({tag + n: g for n, g in zip(hp.RULE_NAMES, grads)})
    return res, [geom, binning, img]


def _raster_case(name):
    """The inputs (helpers.inputs_of) of a scene, asserted ON THE CPU ORACLE to have the structure it is here for."""
    if name in ("scale_rot_sh", "async"):
        d = hp.inputs_of(_scene_a(), "scale_rot")
    elif name == "precomp_colors":
        d = hp.inputs_of(_scene_a(), "precomp", colors=True)
    elif name == "raw_lbs":
        d = hp.inputs_of(_scene_a(), "lbs")
    elif name == "heavy_and_empty_tiles":
        d = hp.inputs_of(_stacked_scene(2500, W=70, H=50, spread=0.25, scale=0.12), "precomp")
    else:
        s = scenes.config1(P=250, W=70, H=50)
        s.means3D[:, 2] -= 10.0                                           # all behind the camera
        d = hp.inputs_of(s, "scale_rot", bg=[0.1, 0.5, 0.9])
    fw = hp.oracle_forward(d)
    if name == "heavy_and_empty_tiles":
        n = fw.ranges[:, 1].astype(np.int64) - fw.ranges[:, 0].astype(np.int64)
        assert (n == 0).any() and (n >= 128).any()
    elif name == "all_culled":
        assert fw.num_rendered == 0
    else:
        assert d.P % 64 != 0 and (np.asarray(fw.radii) == 0).mean() >= 0.25 and fw.num_rendered > 0
    return d


@pytest.mark.parametrize("name", ["scale_rot_sh", "precomp_colors", "raw_lbs", "heavy_and_empty_tiles", "all_culled"])
def test_rasterizer_forward_and_backward(gpu, hip_lib, name):
    """``_C.rasterize_gaussians`` then ``_C.rasterize_gaussians_backward`` under the same poison: image, depth, alpha, radii, R and every
    returned gradient.  Gradient rows of culled Gaussians must come out as zeros, pixels of empty tiles as background, and the count /
    status / header words of the three buffers must be set before they are read.
      scale_rot_sh    scales + rotations + SH, no incoming depth gradient, all_outputs=True (dL_dconic, dL_dcolors, dL_dcov3D are written)
      precomp_colors  the same scene with cov3D_precomp + colors_precomp
      raw_lbs         raw_flags = 7 with per-Gaussian transforms; the raw backward gets the raw opacities
      heavy_and_empty_tiles   2500 Gaussians piled on a few tiles of a 70 x 50 image: lists of >= 128 entries next to an empty tile
      all_culled      R == 0: the image is the background and every gradient is exactly +0"""
    d = _raster_case(name)
    raw = name == "raw_lbs"
    first = under_fills(gpu, lambda: _raster_inputs(d, gpu, raw=raw, depth_grad=name != "scale_rot_sh"),
                        lambda a: _raster_run(d, a, raw_flags=7 if raw else 0, all_outputs=name == "scale_rot_sh"))
    assert {"dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations"} <= first.keys()
    if name == "scale_rot_sh":
        assert {"dL_dcolors", "dL_dcov3D"} <= first.keys()
    if raw:
        assert "dL_dtransforms" in first
    if name == "all_culled":
        assert first["R"] == 0 and not bool(first["radii"].any())
        assert torch.equal(first["color"], d.bg.reshape(3, 1, 1).expand(3, d.H, d.W))
        for n in hp.RULE_NAMES:
            assert n not in first or _plus_zero(first[n]), n
    else:
        culled = first["radii"] == 0
        assert bool(culled.any()) or name == "heavy_and_empty_tiles"
        for n in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dmeans2D"):
            if first[n].numel():
                assert _plus_zero(first[n][culled]), n


def test_rasterizer_asynchronous_forward_never_reads_the_slack(gpu, hip_lib):
    """The asynchronous forward on a private RasterContext: the synchronous call that learns the capacity, a frame at the learned
    capacity, and one at capacity = 4 x needed -- its binning buffer is then mostly slack, which must never be read.  Each with its
    backward; the frame state is the context's own zero-filled block."""
    from moss_amd.diff_gaussian_rasterization import _C
    d = _raster_case("async")

    def run(a):
        cx = _C.RasterContext()
        cx.set_async(True)
        res, also = {}, []
        for tag in ("learn_", "learned_", "slack_"):
            if tag == "slack_":
                cx.capacity = 4 * needed
            r, b = _raster_run(d, a, tag=tag, context=cx)
            cx.check_status()                                             # (raises if the frame overflowed or was dropped)
            needed = int(cx.last_needed)
            res.update(r); also += b
            res[tag + "needed"] = needed
        assert needed > 0 and cx.capacity == 4 * needed and cx.read_dropped_frames() == 0
        return res, also

    first = under_fills(gpu, lambda: _raster_inputs(d, gpu), run)
    for k in ("color", "alpha", "radii", "dL_dmeans3D", "dL_dsh"):        # the same frame three times
        assert _same(first["learn_" + k], first["learned_" + k]) and _same(first["learn_" + k], first["slack_" + k]), k


# ---------------------------------------------------------------- activations
@pytest.mark.parametrize("P,K,unused", [(4097, 16, False), (5, 1, False), (4097, 16, True)])
def test_activate_gaussians(gpu, hip_lib, P, K, unused):
    """``activate_gaussians`` forward + backward without a bucket: the five outputs and the six raw-parameter gradients.  ``unused``: the
    scaling and rotation outputs take no part in the loss, so their gradients come through the kernel's null path as zeros."""
    from moss_amd.activations import activate_gaussians
    names = ("xyz", "dc", "rest", "opa", "scl", "rot")

    def prepare():
        a = _raw_params(P, K, gpu)
        g = torch.Generator().manual_seed(9)
        a["w"] = [torch.randn(*s, generator=g).to(gpu) for s in ((P, 3), (P, K, 3), (P, 1), (P, 3), (P, 4))]
        return a

    def run(a):
        outs = activate_gaussians(*[a[k] for k in names])
        used = (0, 1, 2) if unused else range(5)
        sum((outs[i] * a["w"][i]).sum() for i in used).backward()
        res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
        res.update({"d_" + k: a[k].grad for k in names if a[k].numel()})
        return res, []

    first = under_fills(gpu, prepare, run)
    assert all(("d_" + k) in first for k in names if k != "rest" or K > 1)
    if unused:
        assert _plus_zero(first["d_scl"]) and _plus_zero(first["d_rot"])


# ---------------------------------------------------------------- losses
def _blob_frame(H, W, blobs=2):
    """The masked two-blob frame of test_gpu_ops.py::test_fused_loss_on_masked_frames_with_empty_tiles."""
    g = torch.Generator().manual_seed(9)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    m = torch.zeros(H, W)
    for k in range(blobs):
        cx, cy, r = (0.3 + 0.37 * k) * W, (0.45 + 0.2 * k) * H, 0.17 * min(H, W)
        m = torch.maximum(m, ((xx - cx) ** 2 + ((yy - cy) * 0.8) ** 2 < r * r).float())
    img = torch.rand(3, H, W, generator=g) * m
    gt = torch.rand(3, H, W, generator=g) * torch.roll(m, shifts=(3, -5), dims=(0, 1))
    alpha = torch.rand(1, H, W, generator=g) * m
    return img, alpha, gt, m[None].clone()


def _dense_frame(H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(3, H, W, generator=g); gt = scenes.synthetic_target(H, W)
    alpha = torch.rand(1, H, W, generator=g); mask = (torch.rand(1, H, W, generator=g) > 0.5).float()
    return img, alpha, gt, mask


def _rect_region(H, W, rect, gpu, seed=11):
    """The mask of test_gpu_ops.py::test_fused_moss_loss_matches_torch_expression: an ellipse with holes whose bounding box is ``rect``."""
    from moss_amd.loss import ViewRegion
    x, y, w, h = rect
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    bound = ((((xx - (x + (w - 1) / 2)) / (w / 2)) ** 2 + ((yy - (y + (h - 1) / 2)) / (h / 2)) ** 2) <= 1.0)
    bound &= torch.rand(H, W, generator=g) > 0.02
    bound[y, x:x + w] = True; bound[y + h - 1, x:x + w] = True; bound[y:y + h, x] = True; bound[y:y + h, x + w - 1] = True
    region = ViewRegion(bound[None].to(torch.uint8).to(gpu))
    assert region.xywh == rect
    return region


@pytest.mark.parametrize("case", ["masked_160x200", "dense_70x100", "moss_roi_96x96", "ssim_70x100", "s3im_45x70", "s3im_roi_97x131"])
def test_loss_ops(gpu, hip_lib, case):
    """Value and gradients (image; alpha where the op takes one) of ``training_loss_fused`` (a masked frame whose empty tiles skip the
    filters, and a dense one), ``training_loss_moss_fused`` (rect (37, 41, 11, 9) in 96 x 96), ``ssim_fused``, ``s3im_fused`` and
    ``s3im_loss_roi_fused`` (repeat_time 3).  The losses are multiplied by 1.0 before backward(), so the gradient images the forward
    left in ``torch.empty`` memory are scaled by the incoming gradient and everything unwritten in them would show."""
    from moss_amd import loss as L

    def prepare():
        a = {}
        if case == "masked_160x200":
            img, alpha, gt, mask = _blob_frame(160, 200)
        elif case == "moss_roi_96x96":
            img, alpha, gt, mask = _dense_frame(96, 96, seed=11)
            a["region"] = _rect_region(96, 96, (37, 41, 11, 9), gpu)
        elif case == "s3im_45x70":
            img, alpha, gt, mask = _dense_frame(45, 70)
        elif case == "s3im_roi_97x131":
            img, alpha, gt, mask = _dense_frame(97, 131)
            a["region"] = _rect_region(97, 131, (20, 13, 60, 50), gpu)
        else:
            img, alpha, gt, mask = _dense_frame(70, 100)
        a.update(x=img.to(gpu).requires_grad_(True), al=alpha.to(gpu).requires_grad_(True), gt=gt.to(gpu), mask=mask.to(gpu))
        return a

    def run(a):
        with_alpha = case in ("masked_160x200", "dense_70x100", "moss_roi_96x96")
        if case == "moss_roi_96x96":
            v = L.training_loss_moss_fused(a["x"], a["al"], a["gt"], a["mask"], a["region"])
        elif with_alpha:
            v = L.training_loss_fused(a["x"], a["al"], a["gt"], a["mask"])
        elif case == "ssim_70x100":
            v = L.ssim_fused(a["x"].unsqueeze(0), a["gt"].unsqueeze(0))
        elif case == "s3im_45x70":
            v = L.s3im_fused(a["x"].unsqueeze(0), a["gt"].unsqueeze(0), repeat_time=3)
        else:
            v = L.s3im_loss_roi_fused(a["x"], a["gt"], a["region"], repeat_time=3)
        (v * 1.0).backward()
        return {"value": v.detach(), "d_image": a["x"].grad, "d_alpha": a["al"].grad if with_alpha else None}, []

    first = under_fills(gpu, prepare, run)
    assert bool(torch.isfinite(first["value"])) and bool(first["d_image"].any())


# ---------------------------------------------------------------- deformation and network ops
def test_lbs_deform(gpu, hip_lib):
    """``lbs_deform`` forward + backward at P = 1000, J = 24 with ``x`` and ``want_weights``: T, t, p, w and the gradients of L, A_obs, d, x."""
    from moss_amd import lbs as mlbs
    from tests.test_gpu_lbs import f32, make_case
    P, J = 1000, 24
    c32 = f32(make_case(P, J, 7, "cpu"))
    g = torch.Generator().manual_seed(2)
    cot = [torch.randn(P, *s, generator=g) for s in ((3, 3), (3,), (3,))]

    def prepare():
        a = {k: v.to(gpu) for k, v in c32.items()}
        a["leaves"] = {k: a[k].clone().requires_grad_(True) for k in ("L", "A_obs", "d", "x")}
        a["cot"] = [t.to(gpu) for t in cot]
        return a

    def run(a):
        lv = a["leaves"]
        T, t, p, w = mlbs.lbs_deform(a["ids"], a["W"], lv["L"], a["A_big"], lv["A_obs"], lv["d"], a["R"], a["Th"], x=lv["x"], want_weights=True)
        torch.autograd.backward([T, t, p], a["cot"])
        res = {"T": T.detach(), "t": t.detach(), "p": p.detach(), "w": w.detach()}
        res.update({"d_" + k: v.grad for k, v in lv.items()})
        return res, []

    first = under_fills(gpu, prepare, run)
    assert all(first["d_" + k] is not None for k in ("L", "A_obs", "d", "x"))


def test_smpl_frame_fused(gpu, hip_lib):
    """``smpl_frame_fused`` with ``correct_Rs`` (V = 512, P = 1000 ids): its four outputs and the gradient of ``correct_Rs``."""
    from moss_amd import lbs as mlbs
    P, J, V = 1000, 24, 512
    body = mlbs.synthetic_body_model(V, J, seed=64)
    fr, big = mlbs.synthetic_frame(7, J), mlbs.synthetic_frame(0, J, big_pose=True)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, V, (P,), generator=g)
    cR = mlbs.batch_rodrigues(0.1 * torch.randn(J - 1, 3, generator=g)).contiguous()
    gA, gd = torch.randn(J, 4, 4, generator=g), torch.randn(P, 3, generator=g)

    def prepare():
        up = lambda d: {k: v.to(gpu) for k, v in d.items()}              # noqa: E731
        return dict(body=up(body), fr=up(fr), big=up(big), ids=ids.to(gpu), c=cR.to(gpu).requires_grad_(True), gA=gA.to(gpu), gd=gd.to(gpu))

    def run(a):
        out = mlbs.smpl_frame_fused(a["body"], a["fr"], a["big"], a["ids"], correct_Rs=a["c"])
        torch.autograd.backward([out[1], out[2]], [a["gA"], a["gd"]])
        res = {f"out{i}": t.detach() for i, t in enumerate(out)}
        res["d_correct_Rs"] = a["c"].grad
        return res, []

    first = under_fills(gpu, prepare, run)
    assert len(first) == 5 and bool(first["d_correct_Rs"].any())


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_cross_attention_lbs_fused(gpu, hip_lib, precision):
    """``cross_attention_lbs_fused`` forward + backward at P = 300 (no multiple of the kernels' row tile): the output and the 18 gradients
    (x, Rs, the 16 parameters)."""
    from moss_amd import lbs as mlbs
    from moss_amd import lbs_weights as mlw
    P = 300
    torch.manual_seed(11)
    net0 = mlw.lbs_weight_module()
    g = torch.Generator().manual_seed(5)
    x0 = 0.5 * torch.randn(P, 3, generator=g)
    Rs0 = mlbs.batch_rodrigues(0.2 * torch.randn(23, 3, generator=g)).contiguous()
    cot0 = torch.randn(1, P, 24, generator=g)

    def prepare():
        net = mlw.lbs_weight_module()
        net.load_state_dict(net0.state_dict())
        return dict(net=net.to(gpu), x=x0.to(gpu).requires_grad_(True), Rs=Rs0.to(gpu).requires_grad_(True), cot=cot0.to(gpu))

    def run(a):
        out = mlw.cross_attention_lbs_fused(a["net"], a["x"][None], a["Rs"], precision=precision)
        grads = torch.autograd.grad((out * a["cot"]).sum(), [a["x"], a["Rs"]] + mlw.net_parameters(a["net"]))
        res = {"out": out.detach()}
        res.update({f"g{i}": v for i, v in enumerate(grads)})
        return res, []

    first = under_fills(gpu, prepare, run)
    assert len(first) == 19 and tuple(first["out"].shape) == (1, P, 24)


def test_pose_head_and_matrix_fisher_nll(gpu, hip_lib):
    """``pose_head_fused`` forward + backward (Rs, pose_S, nll and the gradients of the head's parameters) and ``matrix_fisher_nll_fused``
    with its gradient."""
    from moss_amd import lbs as mlbs
    from moss_amd import pose as mpose
    torch.manual_seed(11)
    head0 = mpose.head_module(init_val=0.05)
    g = torch.Generator().manual_seed(5)
    poses = 0.2 * torch.randn(72, generator=g)
    target = mlbs.batch_rodrigues(0.2 * torch.randn(23, 3, generator=g)).contiguous()
    w = torch.randn(23, 3, 3, generator=g)
    F0 = torch.randn(23, 3, 3, generator=g) * 2.0

    def prepare():
        head = mpose.head_module(init_val=0.05)
        head.load_state_dict(head0.state_dict())
        return dict(head=head.to(gpu), poses=poses.to(gpu), target=target.to(gpu), w=w.to(gpu), F=F0.to(gpu).requires_grad_(True))

    def run(a):
        out = mpose.pose_head_fused(a["head"], a["poses"], a["target"])
        grads = torch.autograd.grad((out["Rs"] * a["w"]).sum() + 0.06 * out["nll"].mean(), mpose.head_parameters(a["head"]))
        res = {"Rs": out["Rs"].detach(), "pose_S": out["pose_S"].detach(), "nll": out["nll"].detach()}
        res.update({f"g{i}": v for i, v in enumerate(grads)})
        nll = mpose.matrix_fisher_nll_fused(a["F"], a["target"])
        (nll.mean() * 1.0).backward()
        res.update(fisher_nll=nll.detach(), fisher_dF=a["F"].grad)
        return res, []

    first = under_fills(gpu, prepare, run)
    assert bool(torch.isfinite(first["fisher_nll"]).all()) and bool(first["fisher_dF"].any())


# ---------------------------------------------------------------- densify ops
def test_densify_ops(gpu, hip_lib):
    """On the first golden case of test_gpu_densify_decision.py (P = 600): ``joint_tables``, ``select_clone`` / ``select_split`` /
    ``select_merge`` (mask, the first ``count`` indices, the count), ``clone_rows`` / ``split_rows`` / ``merge_rows`` (the rows, and the
    prune filter merge_rows completes in place), ``prune_mask``; and on 3000 clustered Gaussians ``neighbour_kl`` and ``cal_kl``."""
    from moss_amd import densify as D
    from moss_amd.knn_cuda import knn
    from tests.golden import make_golden_densify as gold
    case = next(iter(gold.CASES))
    g0 = gold.golden_inputs(case)
    g = torch.Generator().manual_seed(6)
    big0 = dict(xyz=_cloud(3000, 5), rotation=torch.randn(3000, 4, generator=g), scaling=-4.0 + 0.5 * torch.randn(3000, 3, generator=g))

    def prepare():
        a = {k: v.to(gpu) for k, v in g0.items()}
        a["accum"], a["denom"], a["lbs_weights"] = a["accum"].reshape(-1), a["denom"].reshape(-1), a["lbs_weights"].reshape(-1, 24)
        a["ids"] = knn(a["xyz"][None], a["xyz"][None], 2)[1][0]
        a["dist"] = knn(a["t_vertices"][None], a["xyz"][None], 1)[0].reshape(-1)
        a["big"] = {k: big0[k].to(gpu) for k in ("xyz", "rotation", "scaling")}
        a["big_ids"] = knn(a["big"]["xyz"][None], a["big"]["xyz"][None], 2)[1][0]
        return a

    def run(a):
        p = [a[k] for k in gold.PARAMS]
        sel = (a["xyz"], a["rotation"], a["scaling"], a["ids"], a["accum"], a["denom"], gold.MAX_GRAD, gold.EXTENT, gold.PERCENT_DENSE)
        res = {"table": D.joint_tables(a["joint_F"], a["denom"])}
        mask, index, n = D.select_clone(*sel, gold.KL_THRESHOLD, surface_mask=a["surface_mask"])
        res.update(clone_mask=mask, clone_index=index, clone_n=n)
        rows = D.clone_rows(index, a["noise_clone"][:n].contiguous(), *p, a["lbs_weights"], a["denom"], res["table"])
        res.update({"clone_" + k: v for k, v in rows.items()})
        mask, index, n = D.select_split(*sel, gold.KL_THRESHOLD)
        res.update(split_mask=mask, split_index=index, split_n=n)
        rows = D.split_rows(index, a["noise_split"][:2 * n].contiguous(), *p)
        res.update({"split_" + k: v for k, v in rows.items()})
        mask, index, n, kl = D.select_merge(*sel, 0.1, want_kl=True)
        res.update(merge_mask=mask.clone(), merge_index=index, merge_n=n, merge_kl=kl)
        rows = D.merge_rows(index, a["ids"], mask, *p)
        res.update({"merge_" + k: v for k, v in rows.items()})
        res["merge_prune_filter"] = mask
        for screen in (None, 20):
            res[f"prune_{screen}"] = D.prune_mask(a["opacity"], a["scaling"], a["max_radii2D"].reshape(-1), a["dist"], gold.MIN_OPACITY, gold.EXTENT, screen)
        b = a["big"]
        res["neighbour_kl"] = D.neighbour_kl(b["xyz"], b["rotation"], torch.exp(b["scaling"]), a["big_ids"])
        res["cal_kl"], res["cal_kl_ids"] = D.cal_kl(b["xyz"], b["rotation"], torch.exp(b["scaling"]))
        return res, []

    first = under_fills(gpu, prepare, run)
    assert min(first["clone_n"], first["split_n"], first["merge_n"]) > 0               # every phase emitted rows
    assert tuple(first["neighbour_kl"].shape) == (3000,) and _same(first["neighbour_kl"], first["cal_kl"])


# ---------------------------------------------------------------- k-NN ops
def _cloud(n, seed, spread=0.02):
    """Points around a few hundred centres: dense clusters and empty space, the cell grid's uneven case."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(200, 3, generator=g) - 0.5
    return centres[torch.randint(0, 200, (n,), generator=g)] + spread * torch.randn(n, 3, generator=g)


def test_knn_ops(gpu, hip_lib):
    """``knn`` brute and grid at k = 1 and 4 over Nr = 3000 references (the grid's workspace -- cell counts, offsets -- comes from
    ``torch.empty``), ``TemplateIndex`` build + query, ``distCUDA2`` at P = 2049."""
    from moss_amd.knn_cuda import TemplateIndex, knn
    from moss_amd.simple_knn._C import distCUDA2
    ref0, q0, pts0 = _cloud(3000, 1), _cloud(2500, 2, 0.05), _cloud(2049, 3)

    def run(a):
        res = {}
        for impl in ("brute", "grid"):
            for k in (1, 4):
                res[f"{impl}{k}_dist"], res[f"{impl}{k}_idx"] = knn(a["ref"][None], a["q"][None], k, impl)
        index = TemplateIndex(a["ref"])
        res["template_ids"], res["template_dist"] = index.query(a["q"], want_dist=True)
        res["dist2"] = distCUDA2(a["pts"])
        return res, [index._index]

    first = under_fills(gpu, lambda: dict(ref=ref0.to(gpu), q=q0.to(gpu), pts=pts0.to(gpu)), run)
    for k in (1, 4):
        assert _same(first[f"brute{k}_idx"], first[f"grid{k}_idx"]) and _same(first[f"brute{k}_dist"], first[f"grid{k}_dist"])


def test_knn_grid_built_under_one_poison_and_queried_under_another(gpu, hip_lib):
    """A ``KnnGrid`` is built once and queried for as long as its references live: built under one fill, queried under a different one."""
    from moss_amd.knn_cuda import KnnGrid
    ref, q = _cloud(3000, 1).to(gpu), _cloud(2500, 2, 0.05).to(gpu)
    got = {}
    for build, query in ((0x00, 0x00), (0xFF, 0x3C), (0x3C, 0xFF), (0x00, 0xFF)):
        gc.collect()
        with hp.poisoned_allocator(gpu, build) as poison:
            grid = KnnGrid(ref)
            poison.assert_owns(grid._ws)
        with hp.poisoned_allocator(gpu, query) as poison:
            dist, idx = grid.query(q, 4)
            poison.assert_owns(dist, idx)
            got[build, query] = (dist.cpu(), idx.cpu())
        del grid, dist, idx
    for key, (dist, idx) in got.items():
        assert _same(dist, got[0, 0][0]) and _same(idx, got[0, 0][1]), key


# ---------------------------------------------------------------- presentation and metrics ops
def test_frames_to_u8(gpu, hip_lib):
    """``frames_to_u8`` at 17 x 33 (no multiple of anything), 3 channels with a region and 4 channels with an alpha."""
    from moss_amd.loss import ViewRegion
    from moss_amd.play import frames_to_u8
    g = torch.Generator().manual_seed(4)
    H, W = 17, 33
    img = torch.rand(3, H, W, generator=g) * 1.4 - 0.2
    alpha = torch.rand(1, H, W, generator=g)
    mask = (torch.rand(1, H, W, generator=g) < 0.6).to(torch.uint8)

    def run(a):
        return {"rgb": frames_to_u8(a["img"], regions=a["region"], fill=1.0), "rgba": frames_to_u8(a["img"], alphas=a["alpha"]),
                "rgb_truncated": frames_to_u8([a["img"], a["img"]], rounding="truncate")[1]}, []

    first = under_fills(gpu, lambda: dict(img=img.to(gpu), alpha=alpha.to(gpu), region=ViewRegion(mask.to(gpu))), run)
    assert tuple(first["rgb"].shape) == (H, W, 3) and tuple(first["rgba"].shape) == (H, W, 4)


def test_posed_vertices_and_bound_masks(gpu, hip_lib):
    """``posed_vertices`` (with joints) and ``bound_masks`` without ``out=``: outputs and workspaces all come from ``torch.empty``.  The
    body, frame and cameras of tests/golden/frame_bounds.npz."""
    from moss_amd import bounds as mb
    from tests.test_frame_bounds_cpu import gen
    z = np.load(os.path.join(ROOT, "tests", "golden", "frame_bounds.npz"))
    body0 = gen.golden_body()
    frame0, pad = gen.golden_frame(0)
    K0, RT0, H, W = torch.tensor(z["K"][0]), torch.tensor(z["RT"][0]), int(z["H"]), int(z["W"])

    def prepare():
        return dict(body={k: v.to(gpu) for k, v in body0.items()}, fr={k: v.to(gpu).contiguous() for k, v in frame0.items()},
                    K=K0.to(gpu), RT=RT0.to(gpu))

    def run(a):
        wv, wb, jt = mb.posed_vertices(a["body"], a["fr"], pad=pad, joints=True)
        bound, rect, corners, flags = mb.bound_masks(wb, a["K"], a["RT"], H, W)
        return dict(world_vertex=wv, world_bound=wb, joints=jt, bound=bound, rect=rect, corners=corners, flags=flags), []

    first = under_fills(gpu, prepare, run)
    assert bool(first["bound"].any()) and set(first["bound"].unique().tolist()) <= {0, 1}


def test_quality_report_add(gpu, hip_lib):
    """``QualityReport.add`` on one 48 x 64 view (its workspace comes from ``torch.empty``): the sums, the per-view values, the filled render."""
    from moss_amd.loss import ViewRegion
    from moss_amd.metrics import QualityReport
    g = torch.Generator().manual_seed(77)
    C, H, W = 3, 48, 64
    image = torch.rand(C, H, W, generator=g) * 1.6 - 0.3
    gt = torch.rand(C, H, W, generator=g)
    mask = (torch.rand(1, H, W, generator=g) < 0.5).float()

    def run(a):
        rep = QualityReport(gpu, C, H, W, a["bg"], per_view_capacity=2)
        out = torch.empty(C, H, W, device=gpu)
        rep.add(a["image"], a["gt"], a["region"], out_image=out)
        rep.add(a["image"], a["gt"], None)
        sums = rep.sums()
        res = {"per_view": rep.per_view(), "out_image": out, "state": rep.state.clone()}
        res.update({"sum_" + k: v for k, v in sums.items()})
        return res, [rep.workspace]

    first = under_fills(gpu, lambda: dict(image=image.to(gpu), gt=gt.to(gpu), region=ViewRegion(mask.to(gpu)), bg=torch.ones(3, device=gpu)), run)
    assert first["sum_n"] == 2 and tuple(first["per_view"].shape) == (2, 3)
