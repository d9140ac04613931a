"""MOSS's LBS-weight network (``CrossAttention_lbs.forward``, nets/mlp_delta_weight_lbs.py:31-54) on the device.

MOSS calls ``pc.cross_attention_lbs(means3D[None], correct_Rs)`` in every training iteration of its pose branch
(gaussian_renderer/__init__.py:72), for all P Gaussians: a 63-channel positional embedding (21 torch ops and a ``cat``), four
``Conv1d(k=1)`` layers of width 128 with a skip, ``Conv1d(128, 24)``, three ``Linear`` layers, two batched matmuls and a softmax.  Here:

* :func:`cross_attention_lbs_fused` -- all of it as ONE HIP launch forward and three backward (C ABI ``moss_lbs_weight_net_forward``
  / ``_backward``, moss_amd/csrc/lbs_weight_net.hip), every layer on the f32-input matrix cores: no host read, no device allocation
  inside the op, capturable, bitwise reproducible.  ``xyz``, ``Rs`` and the 16 parameters the forward reads are inputs of one
  ``autograd.Function``; their ``.grad`` is filled as usual.  ``precision="bf16x3"`` (opt-in) runs the five wide products on the
  bf16-input matrix cores with both operands split in two (``moss_lbs_weight_net_forward_bf16x3`` / ``_backward_bf16x3``).
* :func:`cross_attention_lbs_torch` -- the same mathematics in plain torch (any dtype or device, nothing read back to the host): the
  float64 yardstick of the tests, pinned to the reference's own numbers by tests/golden/lbs_weights_*.npz, and the stand-in for MOSS's
  module in scripts/lbs_weight_net_times.py.  Not a fallback: the fused op has no CPU path.
* :func:`lbs_weight_module` -- a module with the reference's parameter layout, for tests, the timing script and callers without a MOSS
  checkout.

Everything here imports without a GPU.
"""
from __future__ import annotations

import ctypes

import torch

__all__ = ["cross_attention_lbs_fused", "cross_attention_lbs_torch", "lbs_weight_module", "net_parameters", "PARAM_NAMES",
           "PARAM_SHAPES", "UNUSED_NAMES", "NUM_FREQS", "FEATURE_DIM", "PRECISIONS", "split_operand", "preactivations"]

NUM_FREQS = 10
FEATURE_DIM = 24
ROT_DIM = 9
WIDTH = 128
EMBED_DIM = 3 + 6 * NUM_FREQS                                # 63

# the order in which the 16 parameter tensors cross the C ABI: the state_dict keys of MOSS's CrossAttention_lbs that its forward reads
PARAM_NAMES = tuple(f"{m}.{w}" for m in ("bw_linears.0", "bw_linears.1", "bw_linears.2", "bw_linears.3", "bw_fc", "query", "key", "value")
                    for w in ("weight", "bias"))
# as they cross it (a Conv1d(k=1) weight (out, in, 1) is the row-major (out, in) matrix)
PARAM_SHAPES = ((WIDTH, EMBED_DIM), (WIDTH,), (WIDTH, WIDTH), (WIDTH,), (WIDTH, WIDTH), (WIDTH,), (WIDTH, EMBED_DIM + WIDTH), (WIDTH,),
                (FEATURE_DIM, WIDTH), (FEATURE_DIM,), (FEATURE_DIM, FEATURE_DIM), (FEATURE_DIM,), (ROT_DIM, ROT_DIM), (ROT_DIM,),
                (ROT_DIM, ROT_DIM), (ROT_DIM,))
# constructed by the reference, never read by its forward: they cross no boundary and their .grad stays None
UNUSED_NAMES = ("out_layer.weight", "out_layer.bias", "gate_proj.weight", "gate_proj.bias")


# ---- the torch form ---------------------------------------------------------------------------------------------------------------

def _embed(x):
    """``xyz_embedder`` (get_embedder(10), :87-133): the input, then per frequency 2^k three sines followed by three cosines."""
    parts = [x]
    for k in range(NUM_FREQS):
        parts += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(parts, -1)


def _matrix(w):
    return w.reshape(w.shape[0], w.shape[1])                 # Conv1d (out, in, 1) or Linear (out, in)


def split_operand(t, dtype):
    """``(hi, lo)`` of ``t`` in ``t``'s own dtype: ``hi = round(t)`` to ``dtype`` and ``lo = round(t - hi)``."""
    hi = t.to(dtype).to(t.dtype)
    return hi, (t - hi).to(dtype).to(t.dtype)


class _RoundedOperandLinear(torch.autograd.Function):
    """``h @ w.T + b`` with both operands of every product rounded to ``dtype`` and back, in the forward, in the data gradient AND in
    the weight gradient (the backward rounds the incoming gradient too).  The sums are in the tensors' own dtype; the bias gradient is
    the unrounded column sum.  A yardstick only: no kernel computes this."""

    @staticmethod
    def forward(ctx, h, w, b, dtype):
        rounded = lambda t: t.to(dtype).to(t.dtype)                                  # noqa: E731
        hr, wr = rounded(h), rounded(w)
        ctx.save_for_backward(hr, wr)
        ctx.dtype = dtype
        return hr @ wr.t() + b

    @staticmethod
    def backward(ctx, g):
        hr, wr = ctx.saved_tensors
        gr = g.to(ctx.dtype).to(g.dtype)
        return gr @ wr, gr.t() @ hr, g.sum(0), None


class _SplitOperandLinear(torch.autograd.Function):
    """``h @ w.T + b`` with every product ``a b`` replaced by ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)`` (:func:`split_operand`;
    ``lo(a) lo(b)`` is dropped) in the forward (activation x weight), in the data gradient (incoming gradient x weight) AND in the
    weight gradient (incoming gradient x layer input, summed over the points): the backward splits the incoming gradient.  Three
    products each, summed small terms first, in the tensors' own dtype; the bias gradient is the unsplit column sum."""

    @staticmethod
    def forward(ctx, h, w, b, dtype):
        hh, hl = split_operand(h, dtype)
        wh, wl = split_operand(w, dtype)
        ctx.save_for_backward(hh, hl, wh, wl)
        ctx.dtype = dtype
        return ((hl @ wh.t() + hh @ wl.t()) + hh @ wh.t()) + b

    @staticmethod
    def backward(ctx, g):
        hh, hl, wh, wl = ctx.saved_tensors
        gh, gl = split_operand(g, ctx.dtype)
        return ((gl @ wh + gh @ wl) + gh @ wh, (gl.t() @ hh + gh.t() @ hl) + gh.t() @ hh, g.sum(0), None)


def _linear_op(who, operand_dtype, operand_split):
    if operand_split and operand_dtype is None:
        raise ValueError(f"{who}: operand_split needs operand_dtype (the dtype of the two halves)")
    if operand_dtype is None:
        return lambda h, w, b: h @ w.t() + b
    op = _SplitOperandLinear if operand_split else _RoundedOperandLinear
    return lambda h, w, b: op.apply(h, w, b, operand_dtype)


def _trunk(params, x, linear):
    """The five wide layers: q0 (P,24) and the pre-activations of the four hidden layers (P,512)."""
    e = _embed(x)
    h, zs = e, []
    for i in range(4):
        zs.append(linear(h, _matrix(params[f"bw_linears.{i}.weight"]), params[f"bw_linears.{i}.bias"]))
        h = torch.relu(zs[-1])
        if i == 2:
            h = torch.cat((e, h), -1)
    return linear(h, _matrix(params["bw_fc.weight"]), params["bw_fc.bias"]), torch.cat(zs, -1)


def preactivations(params, xyz, operand_dtype=None, operand_split=False):
    """The 512 hidden pre-activations per point (P,512) of :func:`cross_attention_lbs_torch` with the same arguments: where a ReLU
    decides.  For tests that keep their points away from the kinks."""
    return _trunk(params, xyz.reshape(-1, 3), _linear_op("preactivations", operand_dtype, operand_split))[1]


def cross_attention_lbs_torch(params, xyz, Rs, operand_dtype=None, operand_split=False):
    """``CrossAttention_lbs.forward(xyz, Rs)`` in plain torch.  ``params``: a mapping with the module's ``state_dict`` keys
    (:data:`PARAM_NAMES`; others are ignored); ``xyz`` (1,P,3) or (P,3); ``Rs`` (23,3,3) or (1,23,3,3).  Returns (1,P,24).

    ``operand_dtype=torch.bfloat16, operand_split=True``: the arithmetic of ``cross_attention_lbs_fused(precision="bf16x3")`` -- in the
    five wide products (layers 0-3 and ``bw_fc``) both operands are split, ``hi = bf16(a)``, ``lo = bf16(a - hi)``, and every product
    is ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)``, forward, in the data gradient and in the weight gradient
    (``_SplitOperandLinear``); the sums and everything else stay in the tensors' dtype.  In float64 the exact statement of what the
    split kernels compute.  ``operand_dtype`` alone: the operands are ROUNDED instead (``_RoundedOperandLinear``) -- what a plain bf16
    kernel would compute; a yardstick, no kernel does.  The defaults: the function is what it was."""
    x = xyz.reshape(-1, 3)
    q0, _ = _trunk(params, x, _linear_op("cross_attention_lbs_torch", operand_dtype, operand_split))
    M = torch.cat([torch.ones(1, ROT_DIM, dtype=x.dtype, device=x.device), Rs.reshape(-1, ROT_DIM)], 0)      # (24,9)
    Q = q0 @ params["query.weight"].t() + params["query.bias"]
    K = M @ params["key.weight"].t() + params["key.bias"]
    V = M @ params["value.weight"].t() + params["value.bias"]
    att = torch.softmax((Q @ K) / (FEATURE_DIM ** 0.5), -1)
    return (att @ V.t())[None]


def lbs_weight_module():
    """A module with the parameter layout (and ``state_dict`` keys) of MOSS's ``CrossAttention_lbs``, the four tensors its forward never
    reads included, default torch initialisation; ``forward(query, key)`` is :func:`cross_attention_lbs_torch` on its own parameters."""
    from torch import nn

    class LbsWeightNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.bw_linears = nn.ModuleList([nn.Conv1d(EMBED_DIM, WIDTH, 1), nn.Conv1d(WIDTH, WIDTH, 1), nn.Conv1d(WIDTH, WIDTH, 1),
                                             nn.Conv1d(WIDTH + EMBED_DIM, WIDTH, 1)])
            self.bw_fc = nn.Conv1d(WIDTH, FEATURE_DIM, 1)
            self.query = nn.Linear(FEATURE_DIM, FEATURE_DIM)
            self.key = nn.Linear(ROT_DIM, ROT_DIM)
            self.value = nn.Linear(ROT_DIM, ROT_DIM)
            self.out_layer = nn.Linear(FEATURE_DIM, FEATURE_DIM)
            self.gate_proj = nn.Linear(FEATURE_DIM, FEATURE_DIM)

        def forward(self, query, key):
            return cross_attention_lbs_torch(dict(self.named_parameters()), query, key)

    return LbsWeightNet()


# ---- the fused op -----------------------------------------------------------------------------------------------------------------

def net_parameters(net):
    """The 16 parameter tensors of a ``CrossAttention_lbs``-shaped module in :data:`PARAM_NAMES` order; raises if one is missing."""
    named = dict(net.named_parameters())
    missing = [k for k in PARAM_NAMES if k not in named]
    if missing:
        raise ValueError(f"cross_attention_lbs_fused: the module has no parameter {missing[0]} (it needs the layout of MOSS's "
                         "CrossAttention_lbs: bw_linears.0-3, bw_fc, query, key, value)")
    return [named[k] for k in PARAM_NAMES]


PRECISIONS = ("f32", "bf16x3")
_SUFFIX = {"f32": "", "bf16x3": "_bf16x3"}                   # the C entry points of a precision (saved / workspace: the same sizes)


class _LbsWeightNet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Rs, sink, precision, *params):
        from ._lib import LbsWeightNetArgs, call, lib
        dev, P = x.device, int(x.shape[0])
        out = torch.empty((1, P, FEATURE_DIM), dtype=torch.float32, device=dev)
        keep = any(ctx.needs_input_grad)
        saved = torch.empty(lib().moss_lbs_weight_net_saved_bytes(P) // 4 if keep else 0, dtype=torch.float32, device=dev)
        if P > 0:
            a = LbsWeightNetArgs()
            a.P, a.x, a.Rs, a.out, a.saved = P, x.data_ptr(), Rs.data_ptr(), out.data_ptr(), (saved.data_ptr() if keep else None)
            for i, p in enumerate(params):
                a.params[i] = p.data_ptr()
            call("moss_lbs_weight_net_forward" + _SUFFIX[precision], dev, ctypes.byref(a))
        ctx.save_for_backward(x, Rs, saved, *params)
        ctx.sink, ctx.precision = sink, precision
        return out

    @staticmethod
    def backward(ctx, g_out):
        from ._lib import LbsWeightNetBackwardArgs, call, lib
        x, Rs, saved, *params = ctx.saved_tensors
        dev, P = x.device, int(x.shape[0])
        sizes = [3 * P, 23 * 9] + [p.numel() for p in params]
        if P == 0:
            flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        else:
            flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)             # every element is written by the kernels
        g_x, g_Rs, *grads = flat.split(sizes)
        grads = [g.view(p.shape) for g, p in zip(grads, params)]
        if ctx.sink is not None:                                                         # (a sink replaces the parameter's scratch slice)
            from .pose import _sunk
            sunk = [ctx.sink(i) for i in range(len(params))]
            grads = [_sunk(t, g) for t, g in zip(sunk, grads)]
            if P == 0:                                                                   # (no kernel runs: the sinks are zeroed here)
                for t in sunk:
                    if t is not None:
                        t.zero_()
        if P > 0:
            g_out = g_out.reshape(P, FEATURE_DIM).float().contiguous()
            nbytes = lib().moss_lbs_weight_net_workspace_bytes(P)
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a = LbsWeightNetBackwardArgs()
            a.P, a.Rs, a.saved, a.g_out = P, Rs.data_ptr(), saved.data_ptr(), g_out.data_ptr()
            a.g_x, a.g_Rs, a.workspace, a.workspace_bytes = g_x.data_ptr(), g_Rs.data_ptr(), workspace.data_ptr(), nbytes
            for i, (p, g) in enumerate(zip(params, grads)):
                a.params[i], a.grads[i] = p.data_ptr(), g.data_ptr()
            call("moss_lbs_weight_net_backward" + _SUFFIX[ctx.precision], dev, ctypes.byref(a))
        return (g_x.view(P, 3), g_Rs.view(23, 3, 3), None, None, *grads)


def cross_attention_lbs_fused(net, xyz, Rs, grad_sink=None, precision="f32"):
    """MOSS's ``pc.cross_attention_lbs(xyz, Rs)`` as the fused HIP op: one launch forward, three backward.

    ``net``: MOSS's ``CrossAttention_lbs`` instance or anything with the same parameter names and shapes (float32, contiguous, on the
    GPU); ``xyz`` (1,P,3) or (P,3); ``Rs`` (23,3,3) or (1,23,3,3).  Returns (1,P,24).  Gradients flow to ``xyz``, ``Rs`` and the 16
    parameters the forward reads (``out_layer`` / ``gate_proj`` are not read: their ``.grad`` stays ``None``, as with MOSS).

    ``grad_sink``: a callable ``param -> tensor or None`` (the contract of ``GradBucket.sink_for``), asked once per parameter in the
    backward.  Where it returns a tensor (contiguous float32, the parameter's shape) the backward kernels write that parameter's
    gradient THERE and autograd receives that tensor; where it returns None the gradient stays a slice of the op's scratch tensor.  The
    kernels write every element of every weight gradient, so a sink is OVERWRITTEN, not accumulated into (with no Gaussian at all no
    kernel runs and the sinks are zeroed): a sink must hand out each destination at most once per backward pass
    (``GradBucket.sink_for`` does).  The gradients of ``xyz`` and ``Rs`` are not sunk.

    ``precision``: ``"f32"`` (the default: every product exact float32) or ``"bf16x3"`` -- the five wide products (layers 0-3 and
    ``bw_fc``), forward, data gradient and weight gradient, on the bf16-input matrix cores with both operands split,
    ``lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b)``, float32 sums; everything else float32 as before.  It is
    ``cross_attention_lbs_torch(..., operand_dtype=torch.bfloat16, operand_split=True)`` to float32 summation order, bitwise
    reproducible, the same launches.  An unknown name raises ``ValueError`` before anything else is looked at."""
    if precision not in PRECISIONS:
        raise ValueError(f"cross_attention_lbs_fused: precision must be one of {PRECISIONS}, got {precision!r}")
    params = net_parameters(net)
    for name, t in (("xyz", xyz), ("Rs", Rs), *zip(PARAM_NAMES, params)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"cross_attention_lbs_fused runs the HIP kernels of the LBS-weight network: {name} must be a tensor on a "
                               "GPU (cross_attention_lbs_torch is the torch form)")
    dev = xyz.device
    if xyz.shape[-1:] != (3,) or xyz.dim() not in (2, 3) or (xyz.dim() == 3 and xyz.shape[0] != 1):
        raise ValueError(f"cross_attention_lbs_fused: xyz must be (P,3) or (1,P,3), got {tuple(xyz.shape)}")
    if tuple(Rs.shape) not in ((23, 3, 3), (1, 23, 3, 3)):
        raise ValueError(f"cross_attention_lbs_fused: Rs must be (23,3,3) or (1,23,3,3), got {tuple(Rs.shape)}")
    for name, t in (("xyz", xyz), ("Rs", Rs)):
        if t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"cross_attention_lbs_fused: {name} must be float32 on {dev}, got {t.dtype} on {t.device}")
    for name, p, shape in zip(PARAM_NAMES, params, PARAM_SHAPES):
        if tuple(p.shape[:2]) != shape or p.numel() != _numel(shape) or p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
            raise ValueError(f"cross_attention_lbs_fused: {name} must be a contiguous float32 tensor of shape {shape} (a Conv1d weight: "
                             f"{shape + (1,)}) on {dev}, got {tuple(p.shape)} {p.dtype} on {p.device}")
    sink = None if grad_sink is None else (lambda i: grad_sink(params[i]))
    return _LbsWeightNet.apply(xyz.reshape(-1, 3).contiguous(), Rs.reshape(23, 3, 3).contiguous(), sink, precision, *params)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n
