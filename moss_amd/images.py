"""A view's ground truth from its raw image and mask -- on the device, without OpenCV.

MOSS's dataset readers prepare every view on the CPU (``scene/dataset_readers.py:613-654`` ZJU, ``:361-407`` MonoCap, ``:830-868``
DNA-Rendering): ``imread/255``, ``cv2.undistort`` of image and mask, ``image[msk == 0] = background``, ``cv2.resize`` (``INTER_AREA``;
``INTER_NEAREST`` for the mask), ``np.array(image*255.0, dtype=np.byte)`` and later ``PILtoTorch(...)/255``
(``utils/general_utils.py:22-28``).  Here that is two HIP entry points (C ABI ``moss_view_images_prepare`` / ``moss_view_images_load``,
csrc/view_images.hip; the contract is stated in include/moss_raster.h and DESIGN.md):

* :func:`prepare_views` -- once per view: raw bytes in, :class:`ViewImages` out (``gt_u8`` (B,3,H,W), ``bkgd_u8`` (B,H,W): one byte per
  sample, a quarter of the float32 ground truth);
* :meth:`ViewImages.load` -- once per frame change: one launch from the packed bytes to the float32 ``gt_image`` / ``bkgd_mask`` a
  ``MossStep`` reads (capturable: what a ``load_frame`` for ``run_schedule`` calls);
* :func:`prepare_views_torch` -- the same contract in torch ops on any device: the readable statement and the form for callers
  without the library.

The contract is the maintainers' reading of OpenCV 4, NOT OpenCV: the agreement with ``cv2.undistort`` / ``cv2.resize`` is unmeasured
(DESIGN.md lists where the two may differ).  Decoding JPEG / PNG, non-integer area resize, the ``olek_images0812`` variant and the
float64 image path of the DNA-Rendering reader are out of scope.  This module imports without a GPU.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

__all__ = ["prepare_views", "prepare_views_torch", "ViewImages", "MASK_MODES", "SCALES", "MAX_VIEWS_PER_LAUNCH"]

MASK_MODES = ("round", "any")                # (position = the C ABI's mask_mode)  ZJU's uint8 ``msk != 0`` (the byte remap rounds) | MonoCap / DNA-Rendering's float mask/255
SCALES = (1, 2, 4)
MAX_VIEWS_PER_LAUNCH = 8
_TAP_LIMIT = float(1 << 30)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def _host64(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.array(v, dtype=np.float64)


def _lens(who, K, D, B):
    """(K (B,3,3), D (B,5)) host float64 of ``K`` / ``D`` given per view or once for all; the refusals of the C entry point."""
    K = _host64(K)
    if K.size == 9:
        K = np.broadcast_to(K.reshape(1, 3, 3), (B, 3, 3))
    if K.size != 9 * B:
        raise ValueError(f"{who}: K must be (3,3) or ({B},3,3), got {K.shape}")
    K = np.ascontiguousarray(K.reshape(B, 3, 3))
    D = np.zeros((B, 5)) if D is None else _host64(D)
    if D.size == 5:
        D = np.broadcast_to(D.reshape(1, 5), (B, 5))
    if D.size != 5 * B:
        raise ValueError(f"{who}: D must hold k1, k2, p1, p2, k3 once or per view ({B} views), got {D.shape}")
    D = np.ascontiguousarray(D.reshape(B, 5))
    if (K[:, 0, 1] != 0).any():
        raise ValueError(f"{who}: K[0][1] (skew) must be 0")
    if not ((K[:, 0, 0] > 0).all() and (K[:, 1, 1] > 0).all()):
        raise ValueError(f"{who}: fx and fy must be positive")
    return K, D


def _views(who, rgb, mask):
    """``(B, H0, W0, device)`` of ``rgb`` (B,H0,W0,3) and ``mask`` (B,H0,W0), both uint8 on one device."""
    if not isinstance(rgb, torch.Tensor) or not isinstance(mask, torch.Tensor) or rgb.dim() != 4 or rgb.shape[0] < 1 or rgb.shape[3] != 3:
        raise ValueError(f"{who}: rgb must be a (B,H0,W0,3) tensor and mask a (B,H0,W0) tensor, B >= 1")
    B, H0, W0 = (int(v) for v in rgb.shape[:3])
    for t, shape, what in ((rgb, (B, H0, W0, 3), "rgb"), (mask, (B, H0, W0), "mask")):
        if t.dtype != torch.uint8 or tuple(t.shape) != shape or t.device != rgb.device:
            raise ValueError(f"{who}: {what} must be a uint8 tensor of shape {shape} on {rgb.device}, got {t.dtype} {tuple(t.shape)} on "
                             f"{t.device}")
    return B, H0, W0, rgb.device


def _options(who, H0, W0, scale, mask_mode):
    if scale not in SCALES:
        raise ValueError(f"{who}: scale must be one of {SCALES}, got {scale!r} (a non-integer INTER_AREA is out of scope)")
    if H0 % scale or W0 % scale:
        raise ValueError(f"{who}: scale {scale} does not divide {H0} x {W0}")
    if mask_mode not in MASK_MODES:
        raise ValueError(f"{who}: mask_mode must be one of {MASK_MODES}, got {mask_mode!r}")
    if H0 * W0 * 3 >= 2 ** 31:
        raise ValueError(f"{who}: H0 * W0 * 3 must be < 2^31")
    return H0 // scale, W0 // scale


def _scaled_K(K, scale):
    K = K.copy()
    K[:, :2] = K[:, :2] * (1.0 / scale)                      # dataset_readers.py:652: K[:2] = K[:2] * ratio
    return K


def _unit_table(dev):
    """byte -> byte / 255.f, the correctly rounded float32 division (made on the CPU: a GPU division by a scalar may multiply by the
    reciprocal)."""
    return (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)


# ---- the packed ground truth -------------------------------------------------------------------------------------------------------------
class ViewImages:
    """What :func:`prepare_views` returns: ``gt_u8`` (B,3,H,W) and ``bkgd_u8`` (B,H,W) uint8 on the device, ``K`` (B,3,3) host float64
    with rows 0 and 1 multiplied by ``1/scale`` as the reader does (dataset_readers.py:652), ``H``, ``W`` and ``nbytes`` (4 bytes per
    pixel; the float32 tensors they stand for take 16)."""

    def __init__(self, gt_u8, bkgd_u8, K):
        self.gt_u8, self.bkgd_u8, self.K = gt_u8, bkgd_u8, K
        self.H, self.W = int(gt_u8.shape[2]), int(gt_u8.shape[3])
        self.nbytes = gt_u8.numel() + bkgd_u8.numel()

    def __len__(self):
        return int(self.gt_u8.shape[0])

    def load(self, i, gt_image, bkgd_mask):
        """Write view ``i`` as float32 into the caller's ``gt_image`` (3,H,W) and ``bkgd_mask`` (1,H,W): ``u8 / 255.f``, bit for bit
        ``torch.from_numpy(u8) / 255.0``.  ONE launch (C ABI ``moss_view_images_load``), no host read: capturable."""
        from ._lib import ViewImagesLoadArgs, call
        dev = self.gt_u8.device
        if dev.type != "cuda":
            raise RuntimeError("ViewImages.load runs the HIP kernel: it needs GPU tensors (original_image / bkgd_mask work anywhere)")
        n = self.H * self.W
        for t, numel, what in ((gt_image, 3 * n, "gt_image"), (bkgd_mask, n, "bkgd_mask")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != numel or t.device != dev or not t.is_contiguous():
                raise ValueError(f"ViewImages.load: {what} must be a contiguous float32 tensor of {numel} elements on {dev}")
        a = ViewImagesLoadArgs()
        a.H, a.W = self.H, self.W
        a.gt_u8, a.bkgd_u8 = self.gt_u8[i].data_ptr(), self.bkgd_u8[i].data_ptr()
        a.gt_image, a.bkgd_mask = gt_image.data_ptr(), bkgd_mask.data_ptr()
        call("moss_view_images_load", dev, ctypes.byref(a))
        return gt_image, bkgd_mask

    def _float(self, i):
        dev = self.gt_u8.device
        if dev.type == "cuda":
            return self.load(i, torch.empty((3, self.H, self.W), dtype=torch.float32, device=dev),
                             torch.empty((1, self.H, self.W), dtype=torch.float32, device=dev))
        table = _unit_table(dev)
        return table[self.gt_u8[i].long()], table[self.bkgd_u8[i].long()].reshape(1, self.H, self.W)

    def original_image(self, i):
        """A fresh (3,H,W) float32 tensor of view ``i``: a ``Camera``'s ``original_image`` (what ``evaluate_split`` takes as ``gts``)."""
        return self._float(i)[0]

    def bkgd_mask(self, i):
        """A fresh (1,H,W) float32 tensor of view ``i``: a ``Camera``'s ``bkgd_mask``."""
        return self._float(i)[1]

    def fov(self, i):
        """``(FovX, FovY)`` of view ``i`` by the reader's ``focal2fov`` (utils/graphics_utils.py:108-109) on the scaled ``K``
        (dataset_readers.py:656-659)."""
        return (2 * math.atan(self.W / (2 * float(self.K[i, 0, 0]))), 2 * math.atan(self.H / (2 * float(self.K[i, 1, 1]))))


# ---- the fused op ------------------------------------------------------------------------------------------------------------------------
def prepare_views(rgb, mask, K, D=None, scale=2, white_background=False, mask_mode="round"):
    """Raw views to their packed ground truth on the GPU (C ABI ``moss_view_images_prepare``, csrc/view_images.hip; eight views per
    launch, no workspace, no host read).

    ``rgb``: (B,H0,W0,3) uint8 as a decoder delivers it; ``mask``: (B,H0,W0) uint8; both on the GPU, contiguous, at any byte
    address.  ``K`` (3,3) / ``D`` (``k1, k2, p1, p2, k3``; None = no distortion): per view or once for
    all, host values.  ``scale``: 1, 2 or 4 -- the reader's ``image_scaling`` 1, 0.5, 0.25 -- must divide H0 and W0.  ``mask_mode``:
    ``"round"`` (ZJU: the mask is ``msk != 0`` as uint8, whose remap rounds) or ``"any"`` (MonoCap, DNA-Rendering: a float
    ``mask/255``, foreground where the remapped value is not 0).  Returns :class:`ViewImages`.  :func:`prepare_views_torch` states
    the semantics; the two agree on every byte."""
    from ._lib import ViewImagesPrepareArgs, call
    who = "prepare_views"
    B, H0, W0, dev = _views(who, rgb, mask)
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs the HIP kernel: it needs GPU tensors (prepare_views_torch is the torch form)")
    if not rgb.is_contiguous() or not mask.is_contiguous():
        raise ValueError(f"{who}: rgb and mask must be contiguous")
    H, W = _options(who, H0, W0, scale, mask_mode)
    K, D = _lens(who, K, D, B)
    gt_u8 = torch.empty((B, 3, H, W), dtype=torch.uint8, device=dev)
    bkgd_u8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    for k in range(0, B, MAX_VIEWS_PER_LAUNCH):
        a = ViewImagesPrepareArgs()
        m = min(MAX_VIEWS_PER_LAUNCH, B - k)
        a.num_views, a.H0, a.W0, a.scale = m, H0, W0, int(scale)
        a.background, a.mask_mode = int(bool(white_background)), MASK_MODES.index(mask_mode)
        for b in range(m):
            a.rgb[b], a.mask[b] = rgb[k + b].data_ptr(), mask[k + b].data_ptr()
            a.gt_u8[b], a.bkgd_u8[b] = gt_u8[k + b].data_ptr(), bkgd_u8[k + b].data_ptr()
            a.K[b][:] = K[k + b].reshape(-1).tolist()
            a.D[b][:] = D[k + b].tolist()
        call("moss_view_images_prepare", dev, ctypes.byref(a))
    return ViewImages(gt_u8, bkgd_u8, _scaled_K(K, scale))


# ---- the torch statement -------------------------------------------------------------------------------------------------------------------
def prepare_views_torch(rgb, mask, K, D=None, scale=2, white_background=False, mask_mode="round"):
    """:func:`prepare_views` in torch ops, on any device: the readable statement of the contract (include/moss_raster.h) and the form
    for callers without the library.  Every operation is an op of its own, so each rounds on its own."""
    who = "prepare_views_torch"
    B, H0, W0, dev = _views(who, rgb, mask)
    H, W = _options(who, H0, W0, scale, mask_mode)
    K, D = _lens(who, K, D, B)
    f64 = dict(dtype=torch.float64, device=dev)
    col = lambda a: torch.tensor(np.array(a, dtype=np.float64), **f64).reshape(B, 1, 1)            # noqa: E731
    fx, fy, cx, cy = col(K[:, 0, 0]), col(K[:, 1, 1]), col(K[:, 0, 2]), col(K[:, 1, 2])
    k1, k2, p1, p2, k3 = (col(D[:, i]) for i in range(5))
    # 1. the map, in float64
    x = (torch.arange(W0, **f64).reshape(1, 1, W0) - cx) / fx
    y = (torch.arange(H0, **f64).reshape(1, H0, 1) - cy) / fy
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    xy2 = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2 * x2)
    yd = (y * kr + p1 * (r2 + 2 * y2)) + p2 * xy2
    iu, iv = torch.round((fx * xd + cx) * 32), torch.round((fy * yd + cy) * 32)                  # (torch.round: ties to even)
    ok = (iu.abs() < _TAP_LIMIT) & (iv.abs() < _TAP_LIMIT)                                       # (False for NaN and inf)
    qu, qv = torch.where(ok, iu, torch.zeros_like(iu)).long(), torch.where(ok, iv, torch.zeros_like(iv)).long()
    ix, iy = torch.div(qu, 32, rounding_mode="floor"), torch.div(qv, 32, rounding_mode="floor")
    ax, ay = qu - 32 * ix, qv - 32 * iy
    ix, iy = torch.where(ok, ix, torch.full_like(ix, -2)), torch.where(ok, iy, torch.full_like(iy, -2))
    # 2. the taps: (B,H0,W0,4) bytes -- R, G, B, mask -- 0 outside the image
    planes = torch.cat([rgb, mask[..., None]], -1).reshape(B, H0 * W0, 4)
    view = torch.arange(B, device=dev).reshape(B, 1, 1)

    def tap(tx, ty):
        inside = (tx >= 0) & (tx < W0) & (ty >= 0) & (ty < H0)
        got = planes[view, ty.clamp(0, H0 - 1) * W0 + tx.clamp(0, W0 - 1)]
        return torch.where(inside[..., None], got, torch.zeros_like(got)).long()
    t00, t01, t10, t11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    # 3. colour (and the mask of mode "any"), in float32
    unit = _unit_table(dev)
    fx1, fy1 = (ax.float() / 32)[..., None], (ay.float() / 32)[..., None]
    fx0, fy0 = 1 - fx1, 1 - fy1
    w00, w01, w10, w11 = fy0 * fx0, fy0 * fx1, fy1 * fx0, fy1 * fx1
    value = ((unit[t00] * w00 + unit[t01] * w01) + unit[t10] * w10) + unit[t11] * w11           # (B,H0,W0,4)
    if mask_mode == "round":                                                                     # 4. in integers, weights in 1/1024
        fg = lambda t: (t[..., 3] != 0).long()                                                   # noqa: E731
        total = fg(t00) * (32 - ax) * (32 - ay) + fg(t01) * ax * (32 - ay) + fg(t10) * (32 - ax) * ay + fg(t11) * ax * ay
        foreground = total >= 512
        m = foreground.float()
    else:                                                                                        # 5.
        m = value[..., 3]
        foreground = m != 0
    background = torch.full((), 1.0 if white_background else 0.0, dtype=torch.float32, device=dev)
    colour = torch.where(foreground[..., None], value[..., :3], background)                      # 6. the matte
    # the box mean: the balanced pairwise tree over the samples in row-major order
    s = colour.reshape(B, H, scale, W, scale, 3)
    if scale == 1:
        colour = s[:, :, 0, :, 0]
    elif scale == 2:
        colour = ((s[:, :, 0, :, 0] + s[:, :, 0, :, 1]) + (s[:, :, 1, :, 0] + s[:, :, 1, :, 1])) * 0.25
    else:
        rows = [(s[:, :, d, :, 0] + s[:, :, d, :, 1]) + (s[:, :, d, :, 2] + s[:, :, d, :, 3]) for d in range(4)]
        colour = ((rows[0] + rows[1]) + (rows[2] + rows[3])) * 0.0625
    gt_u8 = (colour * 255).to(torch.uint8).permute(0, 3, 1, 2).contiguous()                      # (in [0, 255]: the conversion truncates)
    bkgd_u8 = (m[:, ::scale, ::scale] * 255).to(torch.uint8).contiguous()
    return ViewImages(gt_u8, bkgd_u8, _scaled_K(K, scale))
