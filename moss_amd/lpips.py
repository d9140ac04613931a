"""MOSS's LPIPS term (``loss_fn_vgg(img_pred, img_gt)``, train_ZJU.py:121 and :256; lpipsPyTorch/modules/lpips.py:31-37 with
``net_type='vgg'``) on the device.

A frozen VGG16 (``features[0:30]``: 13 convolutions 3x3 with bias and ReLU, four 2x2 max-pools) is run on both images, the
activations after ReLU 1_2, 2_2, 3_3, 4_3 and 5_3 are normalised per pixel over the channels, and per tap the squared difference goes
through a non-trainable 1x1 convolution to one channel and a spatial mean; the five numbers are summed.  Here:

* :class:`LpipsVGG` -- the frozen weights in the two layouts the kernels read (packed once: forward, and flipped / transposed for the
  data gradient), built from tensors (:meth:`LpipsVGG.from_tensors`) or from the caller's module (:meth:`LpipsVGG.from_module`).
* :func:`lpips_vgg_fused` -- the term as HIP kernels (C ABI ``moss_lpips_vgg_forward`` / ``_backward``, moss_amd/csrc/lpips.hip): both
  images as one batch of two, every wide convolution on the f32-input matrix cores in exact float32, gradient to ``x`` only.  The
  backward reads sign masks, pool winners and the tap gradients the forward left, never a layer input.  No host read, no atomics,
  bitwise reproducible, capturable.
  ``LpipsVGG(..., precision="bf16")`` is the opt-in mixed-precision form of the TRAINING term (``moss_lpips_vgg_forward_bf16`` /
  ``_backward_bf16``), ``precision="bf16x3"`` the split-bf16 (three-product) form between the two (``..._bf16x3``): see
  :class:`LpipsVGG`.  The net carries the choice; the ops take no argument for it.
* :func:`lpips_vgg_roi_fused` -- the same on the ``ViewRegion`` rectangle of two full frames (no crop copies; the offset is read on the
  device, and with ``capacity=`` the crop's size too: one capture serves views whose crops differ in size).
  :func:`crop_capacity` -- the capacity of a dataset's views.
* :class:`LpipsReference`, :func:`lpips_vgg_reference`, :func:`lpips_vgg_roi_reference`, :func:`reference_cache` -- the ground truth's
  tapped activations computed once per camera (``moss_lpips_vgg_reference``) and given to the two ops above in the ground truth's
  place (``moss_lpips_vgg_forward_ref``): the forward then runs VGG16 on one image, not two, and the result is the same.
* :func:`lpips_vgg_torch` -- the same mathematics in plain torch (any dtype or device): the yardstick of the tests and of
  scripts/lpips_times.py.  Not a fallback: the fused op has no CPU path.
* :func:`synthetic_weights` -- VGG16-shaped weights from a seed (a frozen ``numpy.random.RandomState`` stream), for tests, the timing
  script and callers without the 59 MB of pretrained weights.

Everything here imports without a GPU.
"""
from __future__ import annotations

import ctypes
import hashlib
import itertools

import torch

from .loss import region_xywh

__all__ = ["LpipsVGG", "LpipsReference", "lpips_vgg_fused", "lpips_vgg_roi_fused", "lpips_vgg_reference", "lpips_vgg_roi_reference",
           "reference_bytes", "reference_cache", "crop_capacity", "lpips_vgg_torch", "synthetic_weights", "weights_sha256",
           "PRECISIONS", "ALL_PRECISIONS", "CONV_SHAPES", "TAP_CHANNELS", "TAP_AFTER_CONV", "POOL_AFTER_CONV", "SHIFT", "SCALE", "MIN_SIZE"]

_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CONV_SHAPES = tuple((co, ci, 3, 3) for ci, co in zip((3,) + _WIDTHS[:-1], _WIDTHS))
POOL_AFTER_CONV = (1, 3, 6, 9)                            # a 2x2 max-pool follows the ReLU of these convolutions (0-based)
TAP_AFTER_CONV = (1, 3, 6, 9, 12)                         # ReLU 1_2, 2_2, 3_3, 4_3, 5_3: target_layers = [4, 9, 16, 23, 30]
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)                          # BaseNet.mean (lpipsPyTorch/modules/networks.py:40-43)
SCALE = (0.458, 0.448, 0.450)                             # BaseNet.std
MIN_SIZE = 16                                             # four pools: the last tap is at least 1x1
EPS = 1e-10                                               # normalize_activation (lpipsPyTorch/modules/utils.py:5-7)
PRECISIONS = ("f32", "bf16")                              # LpipsVGG(precision=): the operands of the twelve wide convolutions ...
ALL_PRECISIONS = PRECISIONS + ("bf16x3",)                 # ... and the split-bf16 (three-product) form
_SUFFIX = {"f32": "", "bf16": "_bf16", "bf16x3": "_bf16x3"}                          # of the C entry points
_GENERATIONS = itertools.count(1)                         # LpipsVGG.generation: one number per (net, refresh)


# ---- the torch form ---------------------------------------------------------------------------------------------------------------

class _RoundedOperandConv(torch.autograd.Function):
    """``conv2d(h, w, b, padding=1)`` with both operands of every product rounded to ``dtype`` and back (round-to-nearest-even), in
    the forward AND in the data gradient: the backward rounds the incoming gradient and convolves it with the rounded weight.  A plain
    ``.to(dtype)`` would not do: its backward is the identity, and the gradient convolution would see unrounded operands.  The sums
    are in the tensors' own dtype; the weight and the bias get no gradient (they are frozen)."""

    @staticmethod
    def forward(ctx, h, w, b, dtype):
        import torch.nn.functional as F
        rounded = lambda t: t.to(dtype).to(t.dtype)                                  # noqa: E731
        wr = rounded(w)
        ctx.save_for_backward(wr)
        ctx.dtype, ctx.shape = dtype, h.shape
        return F.conv2d(rounded(h), wr, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        (wr,) = ctx.saved_tensors
        return torch.nn.grad.conv2d_input(ctx.shape, wr, g.to(ctx.dtype).to(g.dtype), padding=1), None, None, None


def split_operand(t, dtype):
    """``(hi, lo)`` of ``t`` in ``t``'s own dtype: ``hi = round(t)`` to ``dtype`` and ``lo = round(t - hi)``.  For float32 ``t`` the
    subtraction is exact; ``hi + lo`` carries about twice ``dtype``'s bits of ``t``."""
    hi = t.to(dtype).to(t.dtype)
    return hi, (t - hi).to(dtype).to(t.dtype)


class _SplitOperandConv(torch.autograd.Function):
    """``conv2d(h, w, b, padding=1)`` with every product ``a b`` replaced by ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)``
    (:func:`split_operand`; ``lo(a) lo(b)`` is dropped), in the forward AND in the data gradient: the backward splits the incoming
    gradient and convolves its parts with the split weight.  Three convolutions each way, summed small terms first; the sums are in the
    tensors' own dtype; the weight and the bias get no gradient (they are frozen)."""

    @staticmethod
    def forward(ctx, h, w, b, dtype):
        import torch.nn.functional as F
        wh, wl = split_operand(w, dtype)
        hh, hl = split_operand(h, dtype)
        ctx.save_for_backward(wh, wl)
        ctx.dtype, ctx.shape = dtype, h.shape
        return (F.conv2d(hl, wh, None, padding=1) + F.conv2d(hh, wl, None, padding=1)) + F.conv2d(hh, wh, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        wh, wl = ctx.saved_tensors
        gh, gl = split_operand(g, ctx.dtype)
        gin = torch.nn.grad.conv2d_input
        return (gin(ctx.shape, wh, gl, padding=1) + gin(ctx.shape, wl, gh, padding=1)) + gin(ctx.shape, wh, gh, padding=1), None, None, None


def lpips_vgg_torch(params, x, y, return_terms=False, operand_dtype=None, operand_split=False):
    """``LPIPS.forward(x, y)`` for ``net_type='vgg'`` in plain torch.  ``params``: a mapping with ``conv_weights`` (13 tensors
    (Cout,Cin,3,3)), ``conv_biases`` (13), ``lin_weights`` (5 tensors of C, any shape), ``shift`` and ``scale`` (3 each), all of the
    images' dtype and device; ``x``, ``y`` (3,H,W) or (1,3,H,W).  Returns (1,1,1,1); with ``return_terms`` also the five per-tap
    terms as a (5,) tensor.

    ``operand_dtype=torch.bfloat16``: the arithmetic of ``LpipsVGG(precision="bf16")`` -- in convolutions 2..13 the input, the weight
    and (in the backward) the incoming gradient are rounded to bf16 before they are multiplied; the sums, conv 1_1 and everything else
    stay in the tensors' dtype.  In float64 this is the exact statement of what the bf16 kernels compute.  ``None``: nothing is
    rounded.

    ``operand_split=True`` (with ``operand_dtype=torch.bfloat16``): the arithmetic of ``LpipsVGG(precision="bf16x3")`` -- those operands
    are not rounded but SPLIT, ``hi = bf16(a)``, ``lo = bf16(a - hi)``, and every product is ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)``
    (``_SplitOperandConv``).  In float64 the exact statement of what the split kernels compute.  ``False`` (the default): the function
    is what it was."""
    import torch.nn.functional as F
    if operand_split and operand_dtype is None:
        raise ValueError("lpips_vgg_torch: operand_split needs operand_dtype (the dtype of the two halves)")
    conv_op = _SplitOperandConv if operand_split else _RoundedOperandConv
    shift = params["shift"].reshape(1, 3, 1, 1)
    scale = params["scale"].reshape(1, 3, 1, 1)

    def features(img):
        h = (img.reshape(1, 3, img.shape[-2], img.shape[-1]) - shift) / scale
        taps = []
        for i, (w, b) in enumerate(zip(params["conv_weights"], params["conv_biases"])):
            if operand_dtype is None or i == 0:
                h = torch.relu(F.conv2d(h, w, b, padding=1))
            else:
                h = torch.relu(conv_op.apply(h, w, b, operand_dtype))
            if i in TAP_AFTER_CONV:
                taps.append(h / (torch.sqrt(torch.sum(h ** 2, dim=1, keepdim=True)) + EPS))
            if i in POOL_AFTER_CONV:
                h = F.max_pool2d(h, 2, 2)
        return taps

    fx, fy = features(x), features(y)
    terms = [F.conv2d((a - b) ** 2, lw.reshape(1, -1, 1, 1)).mean((2, 3), True) for a, b, lw in zip(fx, fy, params["lin_weights"])]
    total = torch.sum(torch.cat(terms, 0), 0, True)
    return (total, torch.cat(terms, 0).reshape(5)) if return_terms else total


def synthetic_weights(seed=0):
    """VGG16-shaped LPIPS weights from ``numpy.random.RandomState(seed)``, drawn in this order: per convolution the weight (He-normal,
    std ``sqrt(2 / (9 Cin))``) then the bias (0.05 x normal); then per tap the lin weight (``|normal| / C``).  float32 CPU tensors in
    the mapping :func:`lpips_vgg_torch` takes."""
    import numpy as np
    rs = np.random.RandomState(seed)
    cw, cb, lw = [], [], []
    for co, ci, _, _ in CONV_SHAPES:
        cw.append(torch.from_numpy((rs.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)))
        cb.append(torch.from_numpy((0.05 * rs.standard_normal(co)).astype(np.float32)))
    for c in TAP_CHANNELS:
        lw.append(torch.from_numpy((np.abs(rs.standard_normal(c)) / c).astype(np.float32)))
    return {"conv_weights": cw, "conv_biases": cb, "lin_weights": lw, "shift": torch.tensor(SHIFT, dtype=torch.float32),
            "scale": torch.tensor(SCALE, dtype=torch.float32)}


def weights_sha256(params):
    """SHA-256 over the float32 bytes of the convolution weights and biases (interleaved, in layer order) and the lin weights."""
    h = hashlib.sha256()
    for w, b in zip(params["conv_weights"], params["conv_biases"]):
        h.update(w.detach().float().cpu().contiguous().numpy().tobytes())
        h.update(b.detach().float().cpu().contiguous().numpy().tobytes())
    for w in params["lin_weights"]:
        h.update(w.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def cast_params(params, dtype=None, device=None):
    """The mapping of :func:`lpips_vgg_torch` with every tensor in another dtype / on another device."""
    conv = lambda t: t.to(dtype=dtype, device=device)
    return {k: ([conv(t) for t in v] if isinstance(v, (list, tuple)) else conv(v)) for k, v in params.items()}


# ---- the frozen network as the kernels read it ---------------------------------------------------------------------------------------

def _is_conv(m, k):
    w = getattr(m, "weight", None)
    return isinstance(w, torch.Tensor) and w.dim() == 4 and tuple(w.shape[2:]) == (k, k)


class LpipsVGG:
    """The frozen LPIPS-VGG16 weights on a GPU, packed once into the two layouts of moss_amd/csrc/lpips.hip: per convolution
    ``[Cout][tap][Cin]`` for the forward and ``[Cin][flipped tap][Cout]`` for the data gradient.  The packed copies are this object's
    own; the tensors or the module they came from are only read (:meth:`refresh` reads them again).

    ``precision="f32"`` (the default): every product and sum in float32 -- the only form an evaluation metric may use
    (``metrics.evaluate_views`` refuses any other).  ``precision="bf16"``: in convolutions 2..13, forward and data gradient, both
    operands of every product are rounded to bf16 (nearest even: the weights once, here; the activations and incoming gradients as
    the kernel stages them -- in memory they stay float32) and the sums are float32; conv 1_1 and everything outside the convolutions
    are unchanged (``w_fwd[1:]`` / ``w_bwd[1:]`` are ``torch.bfloat16``, ``[0]`` float32).  It is
    ``lpips_vgg_torch(..., operand_dtype=torch.bfloat16)`` to float32 summation order, bitwise reproducible, and 2.1-2.4x faster
    (256x176: 1.02 against 2.14 ms forward + backward).  What it costs, measured on the CPU with an emulation in torch against exact
    float64, SYNTHETIC weights (``synthetic_weights(0)``; pretrained weights were not measured) -- value relative / gradient relative
    L2 / gradient cosine, and plain float32's gradient relative L2 beside it: uniform noise 37x53 3.8e-4 / 0.058 / 0.9983 (float32:
    1e-6); a person-like crop 101x77 1.1e-2 / 0.23 / 0.974 (0.056); 256x176 1.1e-2 / 0.27 / 0.964 (0.090).  On a person-shaped crop
    float32 itself is 6-9 % from float64 in the gradient (ReLU and pool decisions on the near-black ground flip); bf16 is about three
    times that.  Use it for the training term (weighted 0.5 in MOSS's loss), not for a reported number.

    ``precision="bf16x3"``: the middle -- in the same convolutions every float32 operand ``a`` is SPLIT into two bf16, ``hi = bf16(a)`` and
    ``lo = bf16(a - hi)`` (about 16 bits of ``a``), and every product is ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)``: three exact
    bf16 products summed in float32, ``lo lo`` dropped (the weights are split once, here: ``w_fwd[1:]`` / ``w_bwd[1:]`` are
    ``torch.bfloat16`` of TWICE the elements, a hi plane -- the bf16 net's array bit for bit -- then a lo plane; the activations and
    incoming gradients are split as the kernel stages them).  It is ``lpips_vgg_torch(..., operand_dtype=torch.bfloat16,
    operand_split=True)`` to float32 summation order, bitwise reproducible, and 1.7-1.8x faster than float32 (256x176: 1.20 against
    2.13 ms forward + backward, bf16 1.02; 512x352: 2.64 against 4.66, bf16 2.08).  The same CPU emulation against exact float64, SYNTHETIC
    weights (``synthetic_weights(0)``) -- value relative / gradient relative L2 / gradient cosine, float32's gradient relative L2
    beside it: uniform noise 37x53 6.4e-7 / 3.7e-5 / 1.000000 (float32: 2e-6); a person-like crop 101x77 9.3e-6 / 0.074 / 0.9973
    (0.057); 256x176 3.2e-6 / 0.107 / 0.9942 (0.090).  The value error is a thousand times smaller than bf16's, and on person crops
    the gradient is 1.2-1.3 times float32's own distance from float64 where bf16 is three to four times it.  Still a training term: ``evaluate_views`` takes float32 only."""

    def __init__(self, conv_weights, conv_biases, lin_weights, shift, scale, precision="f32"):
        if precision not in ALL_PRECISIONS:
            raise ValueError(f"LpipsVGG: precision must be one of {ALL_PRECISIONS}, got {precision!r}")
        self.precision = precision
        self._src = (list(conv_weights), list(conv_biases), list(lin_weights), shift, scale)
        cw, cb, lw = self._src[:3]
        if len(cw) != 13 or len(cb) != 13 or len(lw) != 5:
            raise ValueError(f"LpipsVGG: expected 13 convolution weights, 13 biases and 5 lin weights, got {len(cw)}, {len(cb)}, {len(lw)}")
        for i, (w, b, shape) in enumerate(zip(cw, cb, CONV_SHAPES)):
            if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
                raise ValueError(f"LpipsVGG: convolution {i} must have weight {shape} and bias {shape[:1]}, got {tuple(w.shape)} and "
                                 f"{tuple(b.shape)} (VGG16 features[0:30])")
        for i, (w, c) in enumerate(zip(lw, TAP_CHANNELS)):
            if w.numel() != c or (w.dim() == 4 and tuple(w.shape) != (1, c, 1, 1)):
                raise ValueError(f"LpipsVGG: lin weight {i} must hold {c} values ((1,{c},1,1)), got {tuple(w.shape)}")
        if shift.numel() != 3 or scale.numel() != 3:
            raise ValueError("LpipsVGG: shift and scale must hold three values each")
        self.device = cw[0].device
        if self.device.type != "cuda":
            raise RuntimeError("LpipsVGG holds the weights of the HIP kernels: the tensors must be on a GPU (lpips_vgg_torch is the "
                               "torch form)")
        for t in cw + cb + lw + [shift, scale]:
            if t.device != self.device:
                raise ValueError(f"LpipsVGG: every tensor must be on {self.device}, got one on {t.device}")
        self.refresh()

    @classmethod
    def from_tensors(cls, conv_weights, conv_biases, lin_weights, shift, scale, precision="f32"):
        """13 weights (Cout,Cin,3,3), 13 biases, 5 lin weights ((1,C,1,1) or (C,)), shift and scale (3 values each), on one GPU."""
        return cls(conv_weights, conv_biases, lin_weights, shift, scale, precision)

    @classmethod
    def from_module(cls, module, precision="f32"):
        """An :class:`LpipsVGG` of the weights :meth:`find_tensors` finds in the caller's module.  The module stays the caller's: it is
        only read, its ``state_dict`` and checkpoints are untouched."""
        return cls(*cls.find_tensors(module), precision=precision)

    @staticmethod
    def find_tensors(module):
        """``(conv_weights, conv_biases, lin_weights, shift, scale)`` of the caller's LPIPS module.  Finds the weights in the caller's LPIPS module by duck typing, in module order: the 13 convolutions 3x3 and the shift / scale
        buffers under ``module.net`` (``.net.mean`` / ``.net.std`` -- the layout of lpipsPyTorch.LPIPS: ``.net.layers``, ``.lin[i][1]``)
        or under ``module.scaling_layer`` (``.shift`` / ``.scale`` -- the layout of the pip package's ``lpips.LPIPS(net='vgg')``:
        ``.net.slice1..5``, ``.lin0..4.model[-1]``), and the five convolutions 1x1 anywhere else in the module.  The pip package is
        not available where this project is tested, so only the first layout is exercised by the tests; the second follows the
        package's published attribute names.  Anything that is not exactly 13 + 5 convolutions of the expected shapes raises."""
        net = getattr(module, "net", None)
        if net is None or not hasattr(net, "modules"):
            raise ValueError("LpipsVGG.from_module: the module has no .net (expected lpipsPyTorch.LPIPS or lpips.LPIPS(net='vgg'))")
        convs = [m for m in net.modules() if _is_conv(m, 3)]
        inside = set(id(m) for m in net.modules())
        lins = [m for m in module.modules() if _is_conv(m, 1) and id(m) not in inside]
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError(f"LpipsVGG.from_module: found {len(convs)} convolutions 3x3 under .net and {len(lins)} convolutions 1x1 "
                             "outside it; the VGG16 variant of LPIPS has exactly 13 and 5")
        if any(m.bias is None for m in convs) or any(m.bias is not None for m in lins):
            raise ValueError("LpipsVGG.from_module: the 3x3 convolutions need a bias and the lin layers must have none")
        if hasattr(net, "mean") and hasattr(net, "std"):
            shift, scale = net.mean, net.std
        elif hasattr(module, "scaling_layer") and hasattr(module.scaling_layer, "shift") and hasattr(module.scaling_layer, "scale"):
            shift, scale = module.scaling_layer.shift, module.scaling_layer.scale
        else:
            raise ValueError("LpipsVGG.from_module: neither .net.mean / .net.std nor .scaling_layer.shift / .scale")
        return [m.weight for m in convs], [m.bias for m in convs], [m.weight for m in lins], shift, scale

    def refresh(self):
        """Pack the source tensors again (a caller who reloaded its weights), in this net's precision.  Advances ``generation`` (a
        number no other net or refresh has had): an :class:`LpipsReference` made before holds the old weights' activations and is
        refused from here on."""
        from ._lib import call
        self.generation = next(_GENERATIONS)
        cw, cb, lw, shift, scale = self._src
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        self.biases = [f32(b).clone() for b in cb]
        self.lin = [f32(w).reshape(-1).clone() for w in lw]
        self.shift, self.scale = f32(shift).reshape(3).clone(), f32(scale).reshape(3).clone()
        self.w_fwd, self.w_bwd = [], []
        for i, w in enumerate(cw):
            w = f32(w)
            co, ci = int(w.shape[0]), int(w.shape[1])
            prec = self.precision if i > 0 else "f32"                                # (conv 1_1 stays float32 on the VALU)
            planes = 2 if prec == "bf16x3" else 1                                    # (split: a hi plane, then a lo plane)
            fwd = torch.empty(planes * w.numel(), dtype=torch.float32 if prec == "f32" else torch.bfloat16, device=self.device)
            bwd = torch.empty_like(fwd)
            call("moss_lpips_vgg_pack_weights" + _SUFFIX[prec], self.device, ci, co, w.data_ptr(), fwd.data_ptr(), bwd.data_ptr())
            self.w_fwd.append(fwd)
            self.w_bwd.append(bwd)
        return self

    def params(self):
        """The source tensors as the mapping :func:`lpips_vgg_torch` takes (not copies)."""
        cw, cb, lw, shift, scale = self._src
        return {"conv_weights": cw, "conv_biases": cb, "lin_weights": lw, "shift": shift, "scale": scale}


# ---- the fused op -----------------------------------------------------------------------------------------------------------------

def _fill_common(a, net, h, w, frame, rect, capacity):
    a.H, a.W = h, w
    a.frame_H, a.frame_W = frame
    a.rect = None if rect is None else rect.data_ptr()
    a.cap_H, a.cap_W = (0, 0) if capacity is None else capacity


def reference_bytes(h, w):
    """The bytes of an :class:`LpipsReference` block for an ``h`` x ``w`` crop, or for a capacity: the five tapped activation maps of
    one image, 122 floats per crop pixel (22 MB at 256x176).  0 for a size the kernels refuse."""
    from ._lib import lib
    return int(lib().moss_lpips_vgg_reference_bytes(int(h), int(w)))


class LpipsReference:
    """What the ground truth contributes to the term, computed ONCE (:func:`lpips_vgg_reference`, :func:`lpips_vgg_roi_reference`) and
    accepted by :func:`lpips_vgg_fused` / :func:`lpips_vgg_roi_fused` wherever they take the ground-truth tensor: its raw activations
    after ReLU 1_2, 2_2, 3_3, 4_3 and 5_3 (``moss_lpips_vgg_reference`` of include/moss_raster.h states the layout).

    ``block``: one uint8 tensor of :func:`reference_bytes`; ``crop``: the ``(h, w)`` the block holds now (None: nothing loaded yet);
    ``capacity``: the ``(cap_h, cap_w)`` the block is laid out for, or None (laid out for ``crop``); ``precision`` and ``generation``:
    those of the net that made it.  A reference is valid for ONE (weights, precision, crop size or capacity): ``LpipsVGG.refresh()``
    advances the net's generation, and the ops refuse a reference of another precision, generation, device, size or capacity.

    THE SAME RESULT.  Against a reference the term runs on ``x`` alone.  Per row the convolution does not know how many images the
    batch holds; what can differ is the kernel shape, which the launcher picks from the row count -- H W here, 2 H W with two images
    -- and the two shapes sum K in different orders.  So the value, the five terms and the gradient are BIT-IDENTICAL to the two-image
    call of the same net, inputs and capacity whenever every wide layer gets the same shape at M = H W as at M = 2 H W: on a device
    with more than 122 CUs for every crop (or capacity) up to 101x77, where all layers take the 32-row shape either way.  Otherwise
    the two agree to float32 summation order and meet the same bar against float64.  In the bf16 modes the ground truth's
    activations are what that mode's kernels compute for it, as in the two-image call."""

    def __init__(self, block, crop, capacity, precision, generation):
        self.block, self.crop, self.capacity, self.precision, self.generation = block, crop, capacity, precision, generation

    @classmethod
    def empty(cls, net, size, static=False):
        """An unloaded reference on ``net``'s device -- the static buffer of a capture, filled by :meth:`copy_`.  ``size``: the capacity
        ``(cap_h, cap_w)`` (``MossStep(lpips_capacity=)``); with ``static=True`` the one crop size of a call without a capacity."""
        h, w = (int(v) for v in size)
        nbytes = reference_bytes(h, w)
        if nbytes == 0:
            raise ValueError(f"LpipsReference.empty: {h}x{w} is not a size the kernels take (at least {MIN_SIZE}x{MIN_SIZE})")
        block = torch.empty(nbytes, dtype=torch.uint8, device=net.device)
        return cls(block, (h, w) if static else None, None if static else (h, w), net.precision, net.generation)

    @property
    def nbytes(self):
        return self.block.numel()

    @property
    def device(self):
        return self.block.device

    def _layout(self):
        return self.capacity if self.capacity is not None else self.crop

    def copy_(self, other):
        """Load ``other`` into this reference: the block (one device copy, capturable as any ``copy_``) and the host fields.  Both must
        be laid out alike -- one capacity, or without one the same crop size.  This is how a captured step changes frame."""
        if not isinstance(other, LpipsReference):
            raise TypeError(f"LpipsReference.copy_: expected an LpipsReference, got {type(other).__name__}")
        if other.crop is None:
            raise ValueError("LpipsReference.copy_: the source holds nothing yet")
        if self.capacity != other.capacity or self._layout() != other._layout():
            raise ValueError(f"LpipsReference.copy_: the two are laid out differently: capacity {self.capacity} crop {self.crop}, and "
                             f"capacity {other.capacity} crop {other.crop}")
        self.block.copy_(other.block)
        self.crop, self.precision, self.generation = other.crop, other.precision, other.generation
        return self

    def __repr__(self):
        return (f"LpipsReference(crop={self.crop}, capacity={self.capacity}, precision={self.precision!r}, "
                f"generation={self.generation}, nbytes={self.nbytes})")


def _fill_net(a, net, lin=True):
    for i in range(13):
        a.weights[i], a.biases[i] = net.w_fwd[i].data_ptr(), net.biases[i].data_ptr()
    if lin:
        for i in range(5):
            a.lin[i] = net.lin[i].data_ptr()
    a.shift, a.scale = net.shift.data_ptr(), net.scale.data_ptr()


def _make_reference(net, y3, crop, rect, capacity):
    """The reference pass on the (3,FH,FW) ground truth: allocates the block and the workspace, nothing else."""
    from ._lib import LpipsVggReferenceArgs, call, lib
    dev = y3.device
    FH, FW = int(y3.shape[-2]), int(y3.shape[-1])
    h, w = (FH, FW) if crop is None else crop
    L = lib()
    ref = LpipsReference(torch.empty(reference_bytes(*(capacity or (h, w))), dtype=torch.uint8, device=dev), (h, w), capacity,
                         net.precision, net.generation)
    nbytes = int(L.moss_lpips_vgg_workspace_bytes(FH, FW))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = LpipsVggReferenceArgs()
    a.y = y3.data_ptr()
    _fill_common(a, net, h, w, (FH, FW), rect, capacity)
    _fill_net(a, net, lin=False)
    a.reference, a.reference_bytes = ref.block.data_ptr(), ref.nbytes
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_lpips_vgg_reference" + _SUFFIX[net.precision], dev, ctypes.byref(a))
    return ref


class _LpipsVGG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, net, crop, rect, capacity):
        from ._lib import LpipsVggArgs, LpipsVggForwardRefArgs, call, lib
        dev = x.device
        FH, FW = int(x.shape[-2]), int(x.shape[-1])
        h, w = (FH, FW) if crop is None else crop
        keep = ctx.needs_input_grad[0]
        L = lib()
        out = torch.empty((1, 1, 1, 1), dtype=torch.float32, device=dev)
        terms = torch.empty(5, dtype=torch.float32, device=dev)
        nbytes = int(L.moss_lpips_vgg_workspace_bytes(FH, FW))                        # (sized for the frame: any crop of it fits)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        saved = torch.empty(int(L.moss_lpips_vgg_saved_bytes(*(capacity or (h, w)))) if keep else 0, dtype=torch.uint8, device=dev)
        if isinstance(y, LpipsReference):                    # x alone; `saved` is the two-image call's, and so is the backward
            a, entry = LpipsVggForwardRefArgs(), "moss_lpips_vgg_forward_ref"
            a.x, a.reference, a.reference_bytes = x.data_ptr(), y.block.data_ptr(), y.nbytes
        else:
            a, entry = LpipsVggArgs(), "moss_lpips_vgg_forward"
            a.x, a.y = x.data_ptr(), y.data_ptr()
        _fill_common(a, net, h, w, (FH, FW), rect, capacity)
        _fill_net(a, net)
        a.out, a.terms = out.data_ptr(), terms.data_ptr()
        a.saved = saved.data_ptr() if keep else None
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        call(entry + _SUFFIX[net.precision], dev, ctypes.byref(a))
        ctx.net, ctx.crop, ctx.frame, ctx.capacity = net, (h, w), (FH, FW), capacity
        ctx.save_for_backward(saved, rect if rect is not None else torch.empty(0, dtype=torch.int32, device=dev))
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    def backward(ctx, g_out, _g_terms):
        from ._lib import LpipsVggBackwardArgs, call, lib
        saved, rect = ctx.saved_tensors
        net, (h, w), (FH, FW) = ctx.net, ctx.crop, ctx.frame
        dev = saved.device
        g = g_out.reshape(1).to(torch.float32).contiguous()
        d_x = torch.empty((3, FH, FW), dtype=torch.float32, device=dev)             # every element is written by the kernels
        nbytes = int(lib().moss_lpips_vgg_workspace_bytes(FH, FW))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        a = LpipsVggBackwardArgs()
        _fill_common(a, net, h, w, (FH, FW), rect if rect.numel() else None, ctx.capacity)
        for i in range(13):
            a.weights_bwd[i] = net.w_bwd[i].data_ptr()
        a.scale, a.saved, a.g_out, a.dL_dx = net.scale.data_ptr(), saved.data_ptr(), g.data_ptr(), d_x.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        call("moss_lpips_vgg_backward" + _SUFFIX[net.precision], dev, ctypes.byref(a))
        return d_x, None, None, None, None, None


def _check_images(what, net, x, y):
    if not isinstance(net, LpipsVGG):
        raise TypeError(f"{what}: net must be an LpipsVGG (LpipsVGG.from_tensors / from_module), got {type(net).__name__}")
    for name, t in (("x", x), ("y", y)):
        if isinstance(t, LpipsReference):                    # (the ground truth as a reference: _check_reference)
            continue
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{what} runs the HIP kernels of the LPIPS term: {name} must be a tensor on a GPU (lpips_vgg_torch is "
                               "the torch form)")
        if t.dtype != torch.float32 or t.device != net.device:
            raise ValueError(f"{what}: {name} must be float32 on {net.device}, got {t.dtype} on {t.device}")
        if t.dim() == 4 and t.shape[0] != 1:
            raise ValueError(f"{what}: the batch must be 1, got {tuple(t.shape)}")
        if t.dim() not in (3, 4) or t.shape[-3] != 3:
            raise ValueError(f"{what}: {name} must be (3,H,W) or (1,3,H,W), got {tuple(t.shape)}")
    if isinstance(y, LpipsReference):
        return
    if x.shape[-2:] != y.shape[-2:]:
        raise ValueError(f"{what}: the two images differ in size: {tuple(x.shape)} and {tuple(y.shape)}")
    if y.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{what}: y is the ground truth and gets no gradient; detach it")


def _check_reference(what, net, ref, crop, capacity):
    """Host checks of a reference against the call that is about to read it: ``crop`` the call's (h, w), ``capacity`` the call's."""
    if ref.precision != net.precision:
        raise ValueError(f"{what}: the reference was made by a precision={ref.precision!r} net and this net has "
                         f"precision={net.precision!r}; a reference belongs to the precision that made it")
    if ref.generation != net.generation:
        raise ValueError(f"{what}: the reference was made before net.refresh() (or by another net): its generation is "
                         f"{ref.generation}, the net's {net.generation}; make it again")
    if ref.device != net.device:
        raise ValueError(f"{what}: the reference is on {ref.device}, the net on {net.device}")
    if ref.capacity != capacity:
        raise ValueError(f"{what}: the reference is laid out for capacity {ref.capacity} and the call has capacity {capacity}")
    if ref.crop != tuple(crop):
        raise ValueError(f"{what}: the reference holds a {ref.crop[0]}x{ref.crop[1]} crop and the call's is {crop[0]}x{crop[1]}"
                         if ref.crop else f"{what}: the reference holds nothing yet (LpipsReference.empty: copy_ one into it)")


def _apply(net, x, y, crop, rect, return_terms, capacity=None):
    shape = x.shape
    x3 = x.reshape(3, shape[-2], shape[-1]).contiguous()
    y3 = y if isinstance(y, LpipsReference) else y.detach().reshape(3, shape[-2], shape[-1]).contiguous()
    value, terms = _LpipsVGG.apply(x3, y3, net, crop, rect, capacity)
    return (value, terms) if return_terms else value


def lpips_vgg_fused(net, x, y, return_terms=False):
    """MOSS's ``loss_fn_vgg(x, y)`` as the fused HIP op.  ``net``: an :class:`LpipsVGG`; ``x``, ``y``: (3,H,W) or (1,3,H,W) float32 on
    the GPU, H, W >= 16.  Returns (1,1,1,1) float32 (with ``return_terms`` also the five per-tap terms, no gradient).  The gradient
    goes to ``x`` only; a ``y`` that requires grad raises.  Under ``torch.no_grad()``, or when ``x`` needs no gradient, the forward
    keeps nothing.

    ``y`` may be an :class:`LpipsReference` of ``x``'s size made by :func:`lpips_vgg_reference` with this net: half of the forward's
    convolutions are then not run.  The result is the two-image call's, bit for bit where
    the kernel shapes agree (:class:`LpipsReference` states the rule).  A reference of another precision, from before ``net.refresh()``, on
    another device, with a capacity, or of another size than ``x`` raises before anything touches the device."""
    _check_images("lpips_vgg_fused", net, x, y)
    if min(x.shape[-2:]) < MIN_SIZE:
        raise ValueError(f"lpips_vgg_fused: H and W must be >= {MIN_SIZE} (four 2x2 pools), got {tuple(x.shape[-2:])}")
    if isinstance(y, LpipsReference):
        _check_reference("lpips_vgg_fused", net, y, tuple(int(v) for v in x.shape[-2:]), None)
    return _apply(net, x, y, None, None, return_terms)


def _check_truth(what, net, y):
    _check_images(what, net, y, y)
    if min(y.shape[-2:]) < MIN_SIZE:
        raise ValueError(f"{what}: H and W must be >= {MIN_SIZE} (four 2x2 pools), got {tuple(y.shape[-2:])}")
    return y.detach().reshape(3, y.shape[-2], y.shape[-1]).contiguous()


def lpips_vgg_reference(net, y):
    """The :class:`LpipsReference` of the ground truth ``y`` ((3,H,W) or (1,3,H,W) float32 on the GPU) for ``lpips_vgg_fused(net, x,
    ref)``: VGG16 on ``y`` alone (``moss_lpips_vgg_reference``), in the net's precision, keeping the five tapped activation maps and
    nothing else.  No gradient is recorded whatever the mode; it allocates the block and a workspace, reads nothing on the host, and
    is capturable.  What "the same result" means: :class:`LpipsReference`."""
    with torch.no_grad():
        return _make_reference(net, _check_truth("lpips_vgg_reference", net, y), None, None, None)


def lpips_vgg_roi_reference(net, gt_image, region, capacity=None):
    """The :class:`LpipsReference` of the full-frame ground truth on ``region``'s rectangle, for ``lpips_vgg_roi_fused(net, image, ref,
    region, capacity=capacity)``: the crop starts where the two-image call's does (the rectangle's corner, moved so that the crop
    fits the frame).  With ``capacity`` the block is laid out for the capacity and the size is read from ``region.rect`` on the
    device; a reference serves the calls of that one capacity (or, without one, of that one crop size).  What "the same result" means:
    :class:`LpipsReference`."""
    with torch.no_grad():                                    # (as lpips_vgg_reference: nothing is recorded, whatever gt_image requires)
        cap, (h, w) = _roi_sizes("lpips_vgg_roi_reference", net, gt_image, gt_image, region, capacity)
        y3 = gt_image.detach().reshape(3, gt_image.shape[-2], gt_image.shape[-1]).contiguous()
        return _make_reference(net, y3, (h, w), region.rect, cap)


def reference_cache(net, gt_images, regions, capacity=None):
    """``(refs, nbytes)``: one :class:`LpipsReference` per (ground truth, region) -- :func:`lpips_vgg_roi_reference` with ``capacity``
    -- and the bytes they hold together (122 floats per pixel of the capacity, or of each crop: the caller decides how many views to
    keep).  A captured step changes frame by ``step.lpips_reference.copy_(refs[k])``."""
    refs = [lpips_vgg_roi_reference(net, gt, region, capacity) for gt, region in zip(gt_images, regions)]
    return refs, sum(r.nbytes for r in refs)


def crop_capacity(regions):
    """The per-axis maximum ``(h, w)`` over an iterable of ``ViewRegion``: the ``capacity`` of :func:`lpips_vgg_roi_fused` that fits
    every one of them.  Host arithmetic on ``region.xywh``; compute it once, when the dataset is loaded."""
    cap_h = cap_w = 0
    for r in regions:
        _, _, w, h = region_xywh(r, "crop_capacity")
        cap_h, cap_w = max(cap_h, int(h)), max(cap_w, int(w))
    if cap_h == 0:
        raise ValueError("crop_capacity: no regions")
    return cap_h, cap_w


def resolve_capacity(what, capacity, H, W):
    """``capacity`` as ``(cap_h, cap_w)`` ints for an H x W frame: a pair, or ``"frame"``; raises if it is not a size the kernels take."""
    if isinstance(capacity, str):
        if capacity != "frame":
            raise ValueError(f"{what}: capacity must be (cap_h, cap_w) or 'frame', got {capacity!r}")
        return int(H), int(W)
    cap_h, cap_w = (int(v) for v in capacity)
    if min(cap_h, cap_w) < MIN_SIZE or cap_h > H or cap_w > W:
        raise ValueError(f"{what}: the capacity must be at least {MIN_SIZE}x{MIN_SIZE} and fit the {H}x{W} frame, got {cap_h}x{cap_w}")
    return cap_h, cap_w


def _roi_sizes(what, net, image, gt_image, region, capacity):
    """The host checks of a call on a region: the resolved capacity (or None) and the crop's (h, w)."""
    cap = None
    if capacity is not None:                                 # (host arithmetic on the region alone, before anything touches a device)
        cap = resolve_capacity(what, capacity, *region.bound.shape)
        _, _, w, h = region_xywh(region, what)
        if h > cap[0] or w > cap[1]:
            raise ValueError(f"{what}: the region's crop {h}x{w} exceeds the capacity {cap[0]}x{cap[1]}")
    _check_images(what, net, image, gt_image)
    H, W = image.shape[-2:]
    if tuple(region.bound.shape) != (H, W) or region.rect.device != image.device:
        raise RuntimeError(f"{what}: the view's region does not belong to this image")
    _, _, w, h = region_xywh(region, what)
    if min(h, w) < MIN_SIZE or h > H or w > W:
        raise ValueError(f"{what}: the crop must be at least {MIN_SIZE}x{MIN_SIZE} and fit the frame, got {h}x{w}")
    return cap, (int(h), int(w))


def lpips_vgg_roi_fused(net, image, gt_image, region, return_terms=False, capacity=None):
    """``loss_fn_vgg(image[:, y:y+h, x:x+w], gt_image[...])`` for ``(x, y, w, h) = region.xywh`` (train_ZJU.py:115-121) on the FULL
    frames: the gradient is written for the whole ``image`` (zero off the crop), there is no host read and there are no crop copies.
    Capturable.

    ``capacity=None``: the crop's size is the region's NOW and goes into the launches; its offset is read from ``region.rect`` on the
    device.  A replay changes view by ``region.copy_`` among views of that one crop size only.

    ``capacity=(cap_h, cap_w)`` or ``"frame"``: the crop's size is read from ``region.rect`` on the device as well, and the launches and
    buffers are sized for the capacity -- the largest crop the call will see (:func:`crop_capacity` of the dataset's views).  A replay
    changes view by ``region.copy_`` among views of ANY size from ``MIN_SIZE`` up to the capacity; MOSS's bounding rectangles change
    with the pose (scene/dataset_readers.py:432-439, train_ZJU.py:115).  A region that does not fit the capacity raises here; under
    replay nothing on the host sees it, so a caller checks there (``MossStep.check``).  The arithmetic is that of the static call.
    The wide convolution has two kernel shapes which sum K in different orders, picked by the row count -- here the capacity's -- so
    the result is bit-identical to the static call at the same crop exactly when every layer gets the same shape in both: always when
    the crop equals the capacity, and for any capacity up to 64x64 on a device with more than 64 CUs.  Otherwise the two agree to
    float32 summation order and meet the same bar against float64."""
    cap, (h, w) = _roi_sizes("lpips_vgg_roi_fused", net, image, gt_image, region, capacity)
    if isinstance(gt_image, LpipsReference):
        _check_reference("lpips_vgg_roi_fused", net, gt_image, (h, w), cap)
    return _apply(net, image, gt_image, (h, w), region.rect, return_terms, cap)
