"""Evaluation metrics of MOSS's reports -- L1, PSNR, SSIM of a whole split -- accumulated on the device.

MOSS evaluates at iterations 2500 / 2700 / 3000 over the test split (ZJU-MoCap: 22 views x 17 poses = 374) and the train split, and
again in render_ZJU.py; per view (train_ZJU.py:244-253):

    image = torch.clamp(render_output["render"], 0.0, 1.0)
    gt_image = torch.clamp(viewpoint.original_image.to("cuda"), 0.0, 1.0)
    image.permute(1,2,0)[bound_mask[0]==0] = 0 if renderArgs[1].sum().item() == 0 else 1     # a host read per view
    l1_test += l1_loss(image, gt_image).mean().double()
    psnr_test += psnr(image, gt_image).mean().double()       # the mean of the per-channel PSNRs
    ssim_test += ssim(image, gt_image).mean().double()       # five depthwise 11x11 convolutions, the full frame
    lpips_test += loss_fn_vgg(image, gt_image).mean().double()

:func:`quality_torch` is that composition in torch (CPU or GPU, any float dtype).  :class:`QualityReport` computes the same three
numbers with two HIP kernels for up to eight views per launch (C ABI ``moss_eval_metrics``) and keeps the float64 sums on the device:
``add`` / ``add_many`` only queue work (no host read, no allocation: capturable in a hipGraph); ``means()`` reads once.
:func:`evaluate_views` drives a whole split; with ``lpips=`` (a :class:`moss_amd.lpips.LpipsVGG` of the caller's pretrained weights) it
adds the per-view LPIPS from the fused op, else ``out_image`` receives the clamped and filled render a caller's own LPIPS runs on.
"""
from __future__ import annotations

import ctypes

import torch

from . import loss as mloss

__all__ = ["quality_torch", "QualityReport", "evaluate_views", "MAX_VIEWS_PER_LAUNCH"]

MAX_VIEWS_PER_LAUNCH = 8


def _fill_value(background) -> float:
    # `0 if renderArgs[1].sum().item() == 0 else 1` (train_ZJU.py:247): one host read
    return 0.0 if float(torch.as_tensor(background).sum().item()) == 0 else 1.0


def quality_torch(image, gt, bound_mask, background):
    """``(l1, psnr, ssim)`` of one view as 0-d tensors, exactly as train_ZJU.py:244-253 composes utils/loss_utils.py and
    utils/image_utils.py: both images clamped to [0, 1]; the RENDER (only) set to the fill value where ``bound_mask != 1`` (MOSS's masks
    are 0 / 1: its ``bound_mask[0]==0``), fill = 0 on a black ``background``, else 1; ``bound_mask`` None = no fill.  L1 is the mean over
    all C*H*W elements, PSNR the mean of the per-channel PSNRs (+inf for an exact match), SSIM the full frame with zero padding.
    Runs in the images' dtype and on their device: the readable statement of the semantics and the CPU cross-check."""
    image = torch.clamp(image, 0.0, 1.0)
    gt = torch.clamp(gt, 0.0, 1.0)
    if bound_mask is not None:
        H, W = image.shape[-2:]
        image.permute(1, 2, 0)[bound_mask.reshape(H, W) != 1] = _fill_value(background)
    l1 = mloss.l1_loss(image, gt)
    mse = ((image - gt) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)      # utils/image_utils.py:19-21
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    ssim = mloss.ssim(image, gt)
    return l1, psnr, ssim


class QualityReport:
    """Running L1 / PSNR / SSIM sums of a split on the device (C ABI ``moss_eval_metrics``).

    ``QualityReport(device, C, H, W, background)``: the fill value is read from ``background`` here, once (the reference's
    ``.sum().item()``).  ``per_view_capacity`` > 0 keeps the float32 values of the first that many views since the last ``reset()``
    (:meth:`per_view`).  Views are (C,H,W) float32 contiguous tensors on ``device``."""

    def __init__(self, device, C, H, W, background, per_view_capacity=0):
        from ._lib import lib
        L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("QualityReport runs the HIP metric kernels: it needs a GPU device (quality_torch is the torch form)")
        self.C, self.H, self.W = int(C), int(H), int(W)
        self.fill = _fill_value(background)
        nstate = int(L.moss_metrics_state_bytes())
        self.state = torch.zeros(nstate, dtype=torch.uint8, device=self.device)
        self.workspace_bytes = int(L.moss_metrics_workspace_bytes(MAX_VIEWS_PER_LAUNCH, self.C, self.H, self.W))
        if self.workspace_bytes == 0:
            raise ValueError(f"QualityReport: bad image shape {(C, H, W)}")
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=self.device)
        self.per_view_capacity = int(per_view_capacity)
        self._per_view = torch.zeros((max(self.per_view_capacity, 1), 3), dtype=torch.float32, device=self.device)
        # doubles [4..7] of the state block are never touched by the kernels: word 4 holds the caller's LPIPS sum (evaluate_views)
        self.extra = self.state.view(torch.float64)[4:5]

    def reset(self):
        self.state.zero_()

    def _check(self, t, what, dtype=torch.float32, shape=None):
        shape = (self.C, self.H, self.W) if shape is None else shape
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"QualityReport: {what} must be a contiguous {dtype} tensor of shape {shape} on {self.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def add(self, image, gt, region=None, out_image=None):
        """Queue one view.  ``region``: the view's :class:`moss_amd.loss.ViewRegion` (its ``bound``: the render is filled where it is 0)
        or None (no fill); ``out_image`` (optional, (C,H,W) float32): receives the clamped and filled render."""
        self.add_many([(image, gt, region, out_image)])

    def add_many(self, views):
        """Queue views given as tuples ``(image, gt[, region[, out_image]])``, eight per launch, in order."""
        from ._lib import EvalMetricsArgs, call
        views = list(views)
        for k in range(0, len(views), MAX_VIEWS_PER_LAUNCH):
            chunk = views[k:k + MAX_VIEWS_PER_LAUNCH]
            a = EvalMetricsArgs()
            a.num_views, a.C, a.H, a.W = len(chunk), self.C, self.H, self.W
            for b, v in enumerate(chunk):
                image, gt = v[0], v[1]
                region = v[2] if len(v) > 2 else None
                out_image = v[3] if len(v) > 3 else None
                self._check(image, "image")
                self._check(gt, "gt")
                a.image[b], a.gt[b] = image.data_ptr(), gt.data_ptr()
                if region is not None:
                    self._check(region.bound, "region.bound", torch.uint8, (self.H, self.W))
                    a.bound[b] = region.bound.data_ptr()
                if out_image is not None:
                    self._check(out_image, "out_image")
                    a.out_image[b] = out_image.data_ptr()
            a.fill = self.fill
            a.state = self.state.data_ptr()
            a.per_view = self._per_view.data_ptr() if self.per_view_capacity > 0 else None
            a.per_view_capacity = self.per_view_capacity
            a.workspace, a.workspace_bytes = self.workspace.data_ptr(), self.workspace_bytes
            call("moss_eval_metrics", self.device, ctypes.byref(a))

    def _read(self):
        s = self.state.cpu()                                  # the one host read
        f, n = s.view(torch.float64), int(s.view(torch.int64)[3])
        return f, n

    def means(self):
        """``{"l1", "psnr", "ssim", "n"}``: the set means (the float64 sums over the views added since the reset, / n), Python floats."""
        f, n = self._read()
        d = max(n, 1)
        return {"l1": float(f[0]) / d, "psnr": float(f[1]) / d, "ssim": float(f[2]) / d, "n": n}

    def sums(self):
        """The float64 sums ``{"l1", "psnr", "ssim", "extra", "n"}`` as they stand on the device (one host read)."""
        f, n = self._read()
        return {"l1": float(f[0]), "psnr": float(f[1]), "ssim": float(f[2]), "extra": float(f[4]), "n": n}

    def per_view(self):
        """(n, 3) float32 CPU tensor of {l1, psnr, ssim} of the views added since the reset (at most ``per_view_capacity`` rows)."""
        _, n = self._read()
        return self._per_view[:min(n, self.per_view_capacity)].cpu()


def evaluate_views(pc, cameras, gts, regions, bg, transforms=None, translation=None, lpips_fn=None, lpips=None,
                   lpips_references=None):
    """MOSS's ``training_report`` over one split (train_ZJU.py:238-262), the metric part on the device: every view rendered with
    ``render()`` under ``torch.no_grad()`` (the forward-only path), its L1 / PSNR / SSIM added to a :class:`QualityReport`, and -- with
    ``lpips_fn`` -- ``lpips_fn(image, gt_image)`` on the clamped and filled render and the clamped ground truth, accumulated in float64
    on the device.  ``gts``: (3,H,W) float32 images; ``regions``: a :class:`moss_amd.loss.ViewRegion` per view or None (no fill);
    ``transforms`` / ``translation``: one LBS table for all views or a list.  No host read inside the loop; one at the end.
    ``lpips``: a :class:`moss_amd.lpips.LpipsVGG` instead of ``lpips_fn`` -- the term from the fused HIP op
    (:func:`moss_amd.lpips.lpips_vgg_fused`, its forward that keeps nothing), summed in float64 in view order like the others.  The net
    must be a float32 one: reported LPIPS is the float32 term, and a ``precision="bf16"`` net (the training term's mixed-precision
    mode) raises ``ValueError`` before anything is rendered.
    ``lpips_references`` (with ``lpips``): one :class:`moss_amd.lpips.LpipsReference` per view, made by
    ``lpips_vgg_reference(lpips, torch.clamp(gts[i], 0, 1))`` and used instead of the clamped ground truth: evaluation is forward-only,
    so half of every LPIPS call is otherwise VGG16 on an image that never changes.  The same means (``lpips.LpipsReference`` states
    when bit for bit); references of a net that is not float32 raise like the net itself.
    Returns ``{"l1", "psnr", "ssim", "lpips", "n"}``: the reference's four set means (``lpips`` None without ``lpips_fn`` / ``lpips``)."""
    if lpips is not None and getattr(lpips, "precision", "f32") != "f32":
        raise ValueError(f"evaluate_views: reported LPIPS is the float32 term; the net given has precision={lpips.precision!r} "
                         "(build a second LpipsVGG with precision='f32' for evaluation)")
    if lpips_references is not None:
        lpips_references = list(lpips_references)
        if lpips is None:
            raise ValueError("evaluate_views: lpips_references needs lpips= (the LpipsVGG that made them)")
        for r in lpips_references:
            if getattr(r, "precision", None) != "f32":
                raise ValueError(f"evaluate_views: reported LPIPS is the float32 term; a reference given has precision="
                                 f"{getattr(r, 'precision', None)!r}")
    from types import SimpleNamespace

    from .diff_gaussian_rasterization import RasterContext
    from .diff_gaussian_rasterization._C import CapacityOverflow
    from .gaussian_renderer import render
    if lpips is not None:
        if lpips_fn is not None:
            raise ValueError("evaluate_views: give lpips_fn or lpips, not both")
        from .lpips import lpips_vgg_fused
        lpips_fn = lambda image, gt: lpips_vgg_fused(lpips, image, gt)      # noqa: E731
    cameras, gts = list(cameras), list(gts)
    n = len(cameras)
    regions = list(regions) if regions is not None else [None] * n
    if len(gts) != n or len(regions) != n or n == 0:
        raise ValueError("evaluate_views: one ground truth and one region (or None) per camera")
    if lpips_references is not None and len(lpips_references) != n:
        raise ValueError("evaluate_views: one LPIPS reference per camera")
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
    transforms, translation = per(transforms), per(translation)
    dev = pc._xyz.device
    C, H, W = gts[0].shape
    report = QualityReport(dev, C, H, W, bg)
    cx = RasterContext()
    cx.set_async(True)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fused_activations=False,
                           transforms_in_op=transforms[0] is not None, pose_in_op=transforms[0] is not None,
                           raw_parameters_in_op=all(hasattr(pc, a) for a in ("_opacity", "_scaling", "_rotation")), raster_context=cx)
    out_image = torch.empty((C, H, W), dtype=torch.float32, device=dev) if lpips_fn is not None else None
    # the renders are asynchronous (no host read per view): the context learns its binning capacity on the first view, and a view that
    # would overflow it renders nothing -- found after the split (the frame state's sticky counter), and the split is evaluated again
    # with the grown capacity
    for attempt in range(3):
        report.reset()
        try:
            with torch.no_grad():
                for i in range(n):
                    image = render(cameras[i], pc, pipe, bg, transforms=transforms[i], translation=translation[i])["render"]
                    report.add(image, gts[i], regions[i], out_image)
                    if lpips_fn is not None:
                        truth = torch.clamp(gts[i], 0.0, 1.0) if lpips_references is None else lpips_references[i]
                        report.extra += lpips_fn(out_image, truth).mean().double()
            s = report.sums()
            cx.check_status()
            if cx.read_dropped_frames() == 0:
                break
        except CapacityOverflow:
            cx.read_dropped_frames()
        if attempt == 2:
            raise RuntimeError("evaluate_views: views kept overflowing the rasterizer's binning capacity")
    return {"l1": s["l1"] / n, "psnr": s["psnr"] / n, "ssim": s["ssim"] / n, "lpips": s["extra"] / n if lpips_fn is not None else None,
            "n": s["n"]}
