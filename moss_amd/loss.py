"""Photometric losses of the measured training step (host side, torch ops).

Semantics follow the reference's utils/loss_utils.py: ``l1_loss`` (:41-42), ``l2_loss`` (:44-45), ``ssim`` with an
11x11 Gaussian window, sigma 1.5, zero padding, depthwise (:47-87); the step combines them as
``L1 + 0.2 * (1 - SSIM)`` (+ 0.5 * mask L2 on the alpha image), the rasterizer-facing terms of train_ZJU.py:111-131.
Pinned by tests/golden/loss_*.npz (generated from the reference functions); MOSS's own composition -- bound_mask selection for L1 / mask L2,
boundingRect crop for SSIM, train_ZJU.py:108-119 -- is ``training_loss_moss`` (torch) / ``training_loss_moss_fused`` (HIP), pinned by
tests/golden/loss_moss.npz.
"""
from __future__ import annotations

from math import exp

import torch
import torch.nn.functional as F

_WINDOWS = {}


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def _window(window_size: int, channel: int, like: torch.Tensor) -> torch.Tensor:
    key = (window_size, channel, like.device, like.dtype)
    w = _WINDOWS.get(key)
    if w is None:
        g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
        g = (g / g.sum()).unsqueeze(1)
        w2 = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
        w = w2.expand(channel, 1, window_size, window_size).contiguous().to(device=like.device, dtype=like.dtype)
        _WINDOWS[key] = w
    return w


def ssim(img1, img2, window_size=11, size_average=True):
    channel = img1.size(-3)
    window = _window(window_size, channel, img1)
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)


def bounding_rect(bound_mask):
    """cv2.boundingRect(bound_mask) (train_ZJU.py:115) of a (1,H,W) / (H,W) 0/1 mask as (x, y, w, h) Python ints (a host read: do it once
    per view when the view is loaded, like the mask's pixel count)."""
    # (the script casts the mask to uint8 first -- a truncation -- and boundingRect takes the non-zero bytes)
    m = bound_mask.reshape(bound_mask.shape[-2], bound_mask.shape[-1]).to(torch.uint8) != 0
    ys, xs = m.any(1).nonzero().flatten(), m.any(0).nonzero().flatten()
    if ys.numel() == 0:
        return 0, 0, 0, 0
    return int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1)


def training_loss_moss(image, alpha, gt_image, bkgd_mask, bound_mask, rect=None, lambda_dssim=0.2, lambda_mask=0.5, ssim_fn=None):
    """MOSS's own expression, torch ops, line by line (train_ZJU.py:108-119,131): L1 and mask L2 over the pixels of ``bound_mask``
    (1,H,W), SSIM on the crop ``rect`` = boundingRect(bound_mask) of both images.  The reference form :func:`training_loss_moss_fused` is
    tested against."""
    sel = bound_mask.reshape(bound_mask.shape[-2], bound_mask.shape[-1]) == 1          # (`bound_mask[0]==1`, :111)
    ll1 = l1_loss(image.permute(1, 2, 0)[sel], gt_image.permute(1, 2, 0)[sel])
    mask_loss = l2_loss(alpha.reshape(sel.shape)[sel], bkgd_mask.reshape(sel.shape)[sel])
    x, y, w, h = rect if rect is not None else bounding_rect(bound_mask)
    s = (ssim_fn or ssim)(image[:, y:y + h, x:x + w].unsqueeze(0), gt_image[:, y:y + h, x:x + w].unsqueeze(0))
    return ll1 + lambda_mask * mask_loss + lambda_dssim * (1.0 - s)


def training_loss(image, alpha, gt_image, gt_mask, lambda_dssim=0.2, lambda_mask=0.5, ssim_fn=None):
    """L1 + lambda_mask * L2(alpha, mask) + lambda_dssim * (1 - SSIM)  (train_ZJU.py:111-112,119,131).  ``ssim_fn``: the SSIM used
    (default: the torch restatement of the reference's; ``ssim_fused`` = the same value from the HIP kernels)."""
    ll1 = l1_loss(image, gt_image)
    mask_loss = l2_loss(alpha, gt_mask)
    s = (ssim_fn or ssim)(image.unsqueeze(0), gt_image.unsqueeze(0))
    return ll1 + lambda_mask * mask_loss + lambda_dssim * (1.0 - s)


_UNIT = {}


def backward_from_loss(loss):
    """``loss.backward()`` without the two minimal kernels autograd would launch for a root loss (ones_like fill + scaling of the
    loss gradients by 1.0): the unit gradient is a cached constant that the fused loss recognises."""
    one = _UNIT.get(loss.device)
    if one is None:
        one = _UNIT[loss.device] = torch.ones((), dtype=loss.dtype, device=loss.device)
    torch.autograd.backward(loss, grad_tensors=one)


def _is_unit(grad_out):
    """The loss is normally the root of the graph: its incoming gradient is then the constant 1 handed to backward() by
    :func:`backward_from_loss`, recognised by identity -- multiplying by exactly 1.0 would be a no-op kernel."""
    unit = _UNIT.get(grad_out.device)
    return unit is not None and grad_out.data_ptr() == unit.data_ptr()


class _FusedPhotometricLoss(torch.autograd.Function):
    """The two loss kernels (C ABI moss_photometric_loss_weighted; with a ``region`` moss_photometric_loss_roi, MOSS's own
    expression): the four terms [loss, L1, SSIM, mask L2] and the gradient of the loss w.r.t. image and alpha come out of the forward;
    backward only scales the gradient by the incoming one.  Returns term ``term``: 0, the loss, or 2, the mean SSIM (under
    ``lambdas`` = (0, 1, 0) and no alpha the loss is 1 - SSIM, so d SSIM / d image = -dL_dimage)."""

    @staticmethod
    def forward(ctx, image, alpha, gt_image, mask, region, lambdas, terms_out, term):
        from ._lib import call, lib, ptr
        C, H, W = image.shape
        dev = image.device
        image_c, gt_c = image.contiguous(), gt_image.contiguous()
        alpha_c, mask_c = (None, None) if alpha is None else (alpha.contiguous(), mask.contiguous())
        if terms_out is not None:
            if terms_out.shape != (4,) or terms_out.dtype != torch.float32 or terms_out.device != dev or not terms_out.is_contiguous():
                raise RuntimeError("fused loss: terms_out must be 4 contiguous float32 values on the image's device")
            out = terms_out
        else:
            out = torch.empty(4, dtype=torch.float32, device=dev)
        # both gradient images in one buffer: backward scales them by the incoming gradient with ONE kernel
        d_both = torch.empty((C if alpha is None else C + 1, H, W), dtype=torch.float32, device=dev)
        nbytes = int(lib().moss_loss_workspace_bytes(C, H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # (the ROI form takes the region's two pointers after the mask, and is otherwise the weighted form)
        name, where = ("moss_photometric_loss_weighted", ()) if region is None else \
            ("moss_photometric_loss_roi", (region.bound.data_ptr(), region.rect.data_ptr()))
        call(name, dev, C, H, W, image_c.data_ptr(), gt_c.data_ptr(), ptr(alpha_c), ptr(mask_c), *where, *lambdas, out.data_ptr(),
             d_both.data_ptr(), None if alpha is None else d_both[C:].data_ptr(), ws.data_ptr(), nbytes)
        ctx.save_for_backward(d_both)
        ctx.C, ctx.alpha_shape, ctx.negate = C, None if alpha is None else alpha.shape, term == 2
        return out[term]

    @staticmethod
    def backward(ctx, grad_out):
        (d_both,) = ctx.saved_tensors
        if ctx.negate:
            scaled = -grad_out * d_both
        else:
            scaled = d_both if _is_unit(grad_out) else grad_out * d_both
        d_alpha = None if ctx.alpha_shape is None else scaled[ctx.C:].reshape(ctx.alpha_shape)
        return scaled[:ctx.C], d_alpha, None, None, None, None, None, None


def ssim_fused(img1, img2, window_size=11, size_average=True):
    """Drop-in for the reference's ``utils.loss_utils.ssim`` (:47-87) as MOSS calls it (train_ZJU.py:119: two (1,3,h,w) crops, the
    defaults): the same value, the gradient w.r.t. ``img1``, from two HIP kernels instead of five depthwise 11x11 convolutions and
    ~20 elementwise kernels forward plus their autograd mirror (on MI355X through MIOpen: 8 x 177 us per step).  In MOSS:
    ``from moss_amd.loss import ssim_fused as ssim`` (patches/train_ZJU.diff).  float32 GPU tensors, (C,H,W) or (1,C,H,W); the second
    image gets no gradient (MOSS's is the ground truth)."""
    if window_size != 11 or not size_average:
        return ssim(img1, img2, window_size, size_average)       # (other windows / per-image means: the torch expressions)
    if img1.dim() == 4:
        if img1.shape[0] != 1:
            return ssim(img1, img2, window_size, size_average)
        img1, img2 = img1[0], img2[0]
    if not img1.is_cuda or img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise RuntimeError("ssim_fused needs float32 GPU tensors (the product path has no CPU fallback; moss_amd.loss.ssim is the torch form)")
    return _FusedPhotometricLoss.apply(img1, None, img2.detach(), None, None, (0.0, 1.0, 0.0), None, 2)


def training_loss_fused(image, alpha, gt_image, gt_mask, lambda_dssim=0.2, lambda_mask=0.5, terms_out=None):
    """Same value and gradients as :func:`training_loss`, computed by the fused HIP kernels.  ``terms_out`` (optional, 4 floats):
    where the kernels write [loss, L1, SSIM, mask L2] -- e.g. ``GradBucket.loss_terms``, so that the loss travels with the
    gradients in the one all-reduce without a copy; the returned loss is then ``terms_out[0]``."""
    if not image.is_cuda:
        raise RuntimeError("fused loss needs GPU tensors; use training_loss() for the torch reference on CPU")
    return _FusedPhotometricLoss.apply(image, alpha, gt_image, gt_mask, None, (1.0, float(lambda_dssim), float(lambda_mask)), terms_out, 0)


class ViewRegion:
    """What MOSS's loss needs of a view besides the two target images, prepared ONCE when the view is loaded: ``bound`` (H,W) uint8 on
    the device, ``rect`` = 5 int32 on the device (x, y, w, h of cv2.boundingRect(bound_mask), the mask's pixel count).  ``copy_(other)``
    rewrites both in place -- how a step captured in a hipGraph changes view."""

    def __init__(self, bound_mask, rect=None):
        m = (bound_mask.reshape(bound_mask.shape[-2], bound_mask.shape[-1]) == 1)      # the script's selection: `bound_mask[0]==1`
        self.bound = m.to(torch.uint8).contiguous()
        x, y, w, h = rect if rect is not None else bounding_rect(bound_mask)
        self.xywh = (x, y, w, h)
        inside = m[y:y + h, x:x + w]                          # (pixels of the mask outside a caller's rectangle count for nothing)
        self.rect = torch.tensor([x, y, w, h, int(inside.sum())], dtype=torch.int32, device=m.device)

    @classmethod
    def from_device(cls, bound, rect):
        """A region over device buffers that something else fills (``moss_amd.bounds``: C ABI ``moss_bound_mask``): ``bound`` (H,W) uint8
        of 0 / 1 and ``rect`` 5 int32 are wrapped as they are -- no copy, no host read -- so a captured consumer sees what the next launch
        writes there.  ``xywh`` is None until :meth:`read`."""
        if bound.dtype != torch.uint8 or bound.dim() != 2 or not bound.is_contiguous():
            raise ValueError(f"ViewRegion.from_device: bound must be a contiguous (H,W) uint8 tensor, got {bound.dtype} {tuple(bound.shape)}")
        if rect.dtype != torch.int32 or tuple(rect.shape) != (5,) or not rect.is_contiguous() or rect.device != bound.device:
            raise ValueError(f"ViewRegion.from_device: rect must be 5 contiguous int32 on {bound.device}, got {rect.dtype} "
                             f"{tuple(rect.shape)} on {rect.device}")
        self = cls.__new__(cls)
        self.bound, self.rect, self.xywh = bound, rect, None
        return self

    def read(self, rect_host=None):
        """Set ``xywh`` from ``rect`` as it is NOW on the device: one host read (it synchronises), or none with ``rect_host``, the
        five values somebody has read already.  Returns ``self``."""
        x, y, w, h = (int(v) for v in (self.rect.tolist() if rect_host is None else rect_host)[:4])
        self.xywh = (x, y, w, h)
        return self

    def copy_(self, other):
        self.bound.copy_(other.bound)
        self.rect.copy_(other.rect)
        self.xywh = other.xywh
        return self


def region_xywh(region, who):
    """``region.xywh`` for a consumer that needs the rectangle on the host; a region made by ``ViewRegion.from_device`` has none until
    ``region.read()``."""
    if region.xywh is None:
        raise RuntimeError(f"{who}: the region's rectangle has not been read on the host (it wraps device buffers: "
                           "ViewRegion.from_device); call region.read() first -- one host read")
    return region.xywh


def training_loss_moss_fused(image, alpha, gt_image, bkgd_mask, region, lambda_dssim=0.2, lambda_mask=0.5, terms_out=None):
    """``Ll1 + lambda_mask * mask_loss + lambda_dssim * (1 - ssim_loss)`` with the three terms EXACTLY as MOSS forms them
    (train_ZJU.py:108-119,131: bound_mask selection, boundingRect crop) -- :func:`training_loss_moss` -- from two HIP kernels.  ``region``:
    the view's :class:`ViewRegion` (made once per view: the rectangle and the pixel count are host reads).  In MOSS this replaces lines
    :111-119 (patches/train_ZJU.diff keeps them and swaps only ``ssim``; this is the one-call form).  The remaining terms of :131 (lpips,
    s3im, nll) are other subsystems' and are added to the returned loss by the caller."""
    if not image.is_cuda or image.dtype != torch.float32:
        raise RuntimeError("fused loss needs float32 GPU tensors; training_loss_moss() is the torch form")
    if tuple(region.bound.shape) != tuple(image.shape[1:]) or region.bound.device != image.device:
        raise RuntimeError("fused loss: the view's region does not belong to this image")
    return _FusedPhotometricLoss.apply(image, alpha, gt_image, bkgd_mask.to(torch.float32), region,
                                       (1.0, float(lambda_dssim), float(lambda_mask)), terms_out, 0)


# ---------------------------------------------------------------------------------------------------------------------------- S3IM
def s3im(src_vec, tar_vec, repeat_time=10):
    """The reference's ``s3im_fun`` (utils/loss_utils.py:17-38) in torch, any device and dtype: the rows of the (b, C*h*w) images are
    gathered in the order [0 .. b-1] followed by ``repeat_time - 1`` draws of ``torch.randperm(b)`` (the default generator, as the
    reference draws them), laid side by side as a (1, C, h, w * repeat_time) image each, and the loss is ``1 - ssim`` of the two.
    At b = 1 -- MOSS's call, two (1,3,h,w) crops -- every permutation is [0] and nothing is drawn: each pixel appears ``repeat_time``
    times along its row.  At b > 1 the permutations are drawn like the reference's, and, like the reference's reshape, the call then
    fails: the gathered rows hold b times the elements of one (1, C, h, w * repeat_time) image."""
    b, channel, h, w = src_vec.shape
    order = torch.cat([torch.arange(b)] + [torch.randperm(b) for _ in range(repeat_time - 1)])
    if b != 1:
        raise RuntimeError(f"s3im: {b * repeat_time} gathered rows of {channel * h * w} values do not form one "
                           f"(1, {channel}, {h}, {w * repeat_time}) image (the reference's reshape fails the same way for a batch > 1)")

    def widen(v):
        return v.reshape(b, -1)[order].t().reshape(1, channel, h, w * repeat_time)

    return 1.0 - ssim(widen(src_vec), widen(tar_vec))


class _FusedS3IM(torch.autograd.Function):
    """C ABI moss_s3im_loss: ``1 - ssim`` of the widened images and its gradient w.r.t. ``image`` (the ground truth gets none)."""

    @staticmethod
    def forward(ctx, image, gt_image, rect, repeat_time):
        from ._lib import call, lib, ptr
        C, H, W = image.shape
        a, b = image.contiguous(), gt_image.contiguous()
        out = torch.empty(2, dtype=torch.float32, device=a.device)
        d_img = torch.empty((C, H, W), dtype=torch.float32, device=a.device)
        nbytes = int(lib().moss_s3im_workspace_bytes(C, H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        call("moss_s3im_loss", a.device, C, H, W, a.data_ptr(), b.data_ptr(), ptr(rect), int(repeat_time), out.data_ptr(), d_img.data_ptr(),
             ws.data_ptr(), nbytes)
        ctx.save_for_backward(d_img)
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        (d_img,) = ctx.saved_tensors
        return (d_img if _is_unit(grad_out) else grad_out * d_img), None, None, None


def _check_s3im_inputs(image, gt_image, what):
    if not image.is_cuda or image.dtype != torch.float32 or gt_image.dtype != torch.float32:
        raise RuntimeError(f"{what} needs float32 GPU tensors (the product path has no CPU fallback; moss_amd.loss.s3im is the torch form)")
    if gt_image.shape != image.shape or gt_image.device != image.device:
        raise RuntimeError(f"{what}: the two images differ in shape or device")


def s3im_fused(src_vec, tar_vec, repeat_time=10):
    """Drop-in for the reference's ``s3im_fun`` (utils/loss_utils.py:17-38) as MOSS calls it (train_ZJU.py:123: two (1,3,h,w) crops):
    the same value, the gradient w.r.t. ``src_vec``, from two HIP kernels (C ABI moss_s3im_loss) instead of the torch graph on a
    tensor ``repeat_time`` times the crop's width.  float32 GPU tensors, (1,C,h,w) or (C,h,w); ``repeat_time`` 1..16; the target gets no
    gradient (MOSS's is the ground truth).  A batch > 1 goes to :func:`s3im`, the reference's semantics."""
    if src_vec.dim() == 4:
        if src_vec.shape[0] != 1:
            return s3im(src_vec, tar_vec, repeat_time)
        src_vec, tar_vec = src_vec[0], tar_vec[0]
    _check_s3im_inputs(src_vec, tar_vec, "s3im_fused")
    return _FusedS3IM.apply(src_vec, tar_vec.detach(), None, repeat_time)


def s3im_loss_roi_fused(image, gt_image, region, repeat_time=10):
    """``s3im_fun(image[:, y:y+h, x:x+w][None], gt_image[...][None])`` for ``(x, y, w, h) = region.xywh`` (train_ZJU.py:115-123), taken
    on the FULL frames: the crop is read from ``region.rect`` on the device -- no host read, no crop copies -- and the gradient is
    written for the whole ``image`` (zero off the crop).  Capturable in a graph; the view changes by ``region.copy_``."""
    _check_s3im_inputs(image, gt_image, "s3im_loss_roi_fused")
    C, H, W = image.shape
    if tuple(region.bound.shape) != (H, W) or region.rect.device != image.device:
        raise RuntimeError("s3im_loss_roi_fused: the view's region does not belong to this image")
    return _FusedS3IM.apply(image, gt_image.detach(), region.rect, repeat_time)
