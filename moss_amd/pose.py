"""MOSS's pose-refinement head and its matrix-Fisher loss term (``Autoregression.forward``, nets/mlp_delta_body_pose.py:56-82, and
``matrix_fisher_nll``, utils/loss_utils.py:283-317) on the device.

MOSS runs, in every training iteration of its pose branch: an MLP 69 -> 128 -> 128 -> 69, a Python loop over the 23 joints (each a
tiny ``Linear`` over the joint's own 3 features and those of its ancestors), its own Rodrigues formula, a batched 3x3 SVD (a host
status check) and the negative log-likelihood of the target rotations under the matrix-Fisher distribution F = U S V^T -- a
determinant taken on the CPU (a device-to-host round trip) and a 512-point quadrature over products of two Bessel polynomials,
three more of them backward.  Here:

* :func:`pose_head_fused` -- all of it, ONE HIP kernel each way (C ABI ``moss_pose_head_forward`` / ``_backward``,
  moss_amd/csrc/pose_head.hip): no host read, no device allocation inside the op, capturable.  The 52 parameters of the caller's
  ``Autoregression`` module are inputs of one ``autograd.Function``; their ``.grad`` is filled as usual.
* :func:`matrix_fisher_nll_fused` -- the loss term alone for general (n,3,3) matrices (C ABI ``moss_matrix_fisher_nll``).
* :func:`autoregression_torch`, :func:`matrix_fisher_nll`, :func:`log_norm_constant` -- the same mathematics in plain torch (any
  dtype or device, nothing read back to the host): the float64 yardstick of the tests, pinned to the reference's own numbers by
  tests/golden/pose_head.npz, and the stand-in for MOSS's chain in scripts/pose_head_times.py.  Not a fallback: the fused ops have no
  CPU path.

Everything here imports without a GPU.
"""
from __future__ import annotations

import ctypes

import torch

from .lbs import SMPL_PARENTS

__all__ = ["pose_head_fused", "matrix_fisher_nll_fused", "autoregression_torch", "matrix_fisher_nll", "log_norm_constant",
           "ancestor_lists", "head_parameters", "head_module", "PARAM_NAMES", "NUM_JOINTS", "SMPL_PARENTS"]

NUM_JOINTS = 23
QUADRATURE_POINTS = 512
# exp(-|x|) I0(x): the polynomial pair of Abramowitz & Stegun 9.8.1 / 9.8.2 in t = x / 3.75 (highest power first, for Horner)
_I0_SMALL = (0.45813e-2, 0.360768e-1, 0.2659732, 1.2067492, 3.0899424, 3.5156229, 1.0)
_I0_LARGE = (0.392377e-2, -0.1647633e-1, 0.2635537e-1, -0.2057706e-1, 0.916281e-2, -0.157565e-2, 0.225319e-2, 0.1328592e-1, 0.39894228)

# the order in which the 52 parameter tensors cross the C ABI: the state_dict keys of MOSS's Autoregression
PARAM_NAMES = tuple(f"block_mlps.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")) + tuple(
    f"fc_pose.{j}.0.{w}" for j in range(NUM_JOINTS) for w in ("weight", "bias"))


# ---- the torch form ---------------------------------------------------------------------------------------------------------------

def ancestor_lists(parents=SMPL_PARENTS):
    """Per non-root joint (joint j here is joint j + 1 of ``parents``) the list of its non-root ancestors, immediate parent first."""
    out = []
    for i in range(1, len(parents)):
        chain, p = [], int(parents[i])
        while p > 0:
            chain.append(p - 1)
            p = int(parents[p])
        out.append(chain)
    return out


def _rodrigues(r):
    """MOSS's ``RodriguesModule``: theta = sqrt(1e-5 + |r|^2), n = r / theta (not a unit vector), R = n n^T (1 - cos) + cos I + sin [n]x."""
    theta = torch.sqrt(1e-5 + (r * r).sum(1))
    n = r / theta[:, None]
    c, s = torch.cos(theta), torch.sin(theta)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    k = 1.0 - c
    rows = (x * x + (1.0 - x * x) * c, x * y * k - z * s, x * z * k + y * s,
            x * y * k + z * s, y * y + (1.0 - y * y) * c, y * z * k - x * s,
            x * z * k - y * s, y * z * k + x * s, z * z + (1.0 - z * z) * c)
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def autoregression_torch(params, poses, parents=SMPL_PARENTS):
    """``Autoregression.forward`` in plain torch.  ``params``: a mapping with the module's ``state_dict`` keys (:data:`PARAM_NAMES`);
    ``poses`` (1,72), the first 3 skipped.  Returns ``{"Rs" (23,3,3), "pose_U", "pose_S", "pose_V"}`` as the reference does."""
    h = poses.reshape(1, -1)[:, 3:]
    for i in (0, 2, 4):
        h = h @ params[f"block_mlps.{i}.weight"].t() + params[f"block_mlps.{i}.bias"]
        if i != 4:
            h = torch.relu(h)
    joint_F = h.reshape(NUM_JOINTS, 3)
    rows = []
    for j, anc in enumerate(ancestor_lists(parents)):
        e = joint_F[[j] + anc].reshape(-1)
        rows.append(params[f"fc_pose.{j}.0.weight"] @ e + params[f"fc_pose.{j}.0.bias"])
    Rs = _rodrigues(torch.stack(rows, 0))
    U, S, Vh = torch.linalg.svd(Rs)
    return {"Rs": Rs, "pose_U": U, "pose_S": S, "pose_V": Vh.transpose(-1, -2)}


def _horner(coeffs, x):
    z = torch.full_like(x, coeffs[0])
    for c in coeffs[1:]:
        z = z * x + c
    return z


def _bessel0_scaled(x):
    """exp(-|x|) I0(x) by the two polynomials, split at |x| <= 3.75 (x = 0 takes the first branch and gives 1)."""
    a = x.abs()
    small = a <= 3.75
    safe = torch.where(small, torch.ones_like(a), a)               # (the large branch is never read where it would divide by 0)
    lo = _horner(_I0_SMALL, (a / 3.75) ** 2) / torch.exp(a)
    hi = _horner(_I0_LARGE, 3.75 / safe) / torch.sqrt(safe)
    return torch.where(small, lo, hi)


def _integrals(si, sj, sk, with_u):
    """0.5 * trapezoid over u in [-1, 1] (512 points, end weights 1/2) of
    I0~((si - sj)(1 - u)/2) I0~((si + sj)(1 + u)/2) exp((sj + sk)(u - 1)) [* u]; si, sj, sk (..., 1)."""
    n = QUADRATURE_POINTS
    u = torch.arange(n, dtype=si.dtype, device=si.device) * (2.0 / (n - 1)) + (-1.0)
    w = torch.ones(n, dtype=si.dtype, device=si.device)
    w[0] = w[-1] = 0.5
    y = _bessel0_scaled((si - sj) * 0.5 * (1 - u)) * _bessel0_scaled((si + sj) * 0.5 * (1 + u)) * torch.exp((sj + sk) * (u - 1))
    if with_u:
        y = y * u
    return 0.5 * ((y * w).sum(-1) * 2.0 / (n - 1))


class _LogNormConstant(torch.autograd.Function):
    """log c(S) = log c~(S) + tr S of the matrix-Fisher distribution (Lee 2018, arXiv:1710.03746, eq. 85-90) by quadrature.  The
    gradient is the quadrature of the ANALYTIC derivative -- dlog c / ds_k = (1 / c~) * the integral with a factor u, over the cyclic
    shift that puts s_k first -- as the reference defines it, not the derivative of the forward's sum."""

    @staticmethod
    def forward(ctx, S):
        c_bar = _integrals(S[:, 1:2], S[:, 2:3], S[:, 0:1], False)
        ctx.save_for_backward(S, c_bar)
        return torch.log(c_bar) + S.sum(1)

    @staticmethod
    def backward(ctx, g):
        S, c_bar = ctx.saved_tensors
        cols = []
        for k in range(3):
            a, b = S[:, (k + 1) % 3], S[:, (k + 2) % 3]
            cols.append(_integrals(torch.maximum(a, b)[:, None], torch.minimum(a, b)[:, None], S[:, k:k + 1], True))
        return torch.stack(cols, 1) / c_bar[:, None] * g[:, None]


def log_norm_constant(S):
    """(N,3) proper singular values, largest first -> (N,) log normalising constants (differentiable as the reference's is)."""
    return _LogNormConstant.apply(S)


def matrix_fisher_nll(pred_F, pred_U, pred_S, pred_V, target_R, overreg=1.005):
    """Drop-in for the reference's ``matrix_fisher_nll`` (same signature, same (N,) result): -<F, R> + overreg * log c(S) with the
    proper singular values s3 * det(U V^T).  The determinant is taken where the tensors live."""
    pred_F, pred_U, pred_V = pred_F.reshape(-1, 3, 3), pred_U.reshape(-1, 3, 3), pred_V.reshape(-1, 3, 3)
    pred_S, target_R = pred_S.reshape(-1, 3), target_R.reshape(-1, 3, 3)
    with torch.no_grad():
        sign = torch.linalg.det(pred_U @ pred_V.transpose(1, 2))
    proper = torch.cat([pred_S[:, :2], pred_S[:, 2:] * sign[:, None]], 1)
    return -(pred_F * target_R).sum((1, 2)) + overreg * log_norm_constant(proper)


# ---- the fused ops ----------------------------------------------------------------------------------------------------------------

def head_parameters(net):
    """The 52 parameter tensors of an ``Autoregression``-shaped module in :data:`PARAM_NAMES` order."""
    mlp, fc = net.block_mlps, net.fc_pose
    out = []
    for i in (0, 2, 4):
        out += [mlp[i].weight, mlp[i].bias]
    for j in range(NUM_JOINTS):
        out += [fc[j][0].weight, fc[j][0].bias]
    return out


def head_module(parents=SMPL_PARENTS, init_val=1e-5):
    """A module with the parameter layout (and ``state_dict`` keys) of MOSS's ``Autoregression`` -- ``block_mlps`` 69 -> 128 -> 128 ->
    69 with ReLUs, ``fc_pose`` one ``Sequential(Linear(3 (1 + ancestors), 3))`` per joint, initialised as MOSS does (uniform
    +-``init_val``, zero bias) -- for tests, the timing script and callers without a MOSS checkout."""
    from torch import nn
    net = nn.Module()
    net.block_mlps = nn.Sequential(nn.Linear(69, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 69))
    net.fc_pose = nn.Sequential(*[nn.Sequential(nn.Linear(3 + 3 * len(a), 3)) for a in ancestor_lists(parents)])
    with torch.no_grad():
        for fc in net.fc_pose:
            fc[0].weight.uniform_(-init_val, init_val)
            fc[0].bias.zero_()
    return net


def _param_shapes(anc):
    shapes = [(128, 69), (128,), (128, 128), (128,), (69, 128), (69,)]
    for a in anc:
        shapes += [(3, 3 + 3 * len(a)), (3,)]
    return shapes


class _PoseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, target_R, overreg, parents, sink, *params):
        from ._lib import POSE_HEAD_SAVED_FLOATS, PoseHeadArgs, call
        dev = poses.device
        nj = NUM_JOINTS
        buf = torch.empty(nj * 13 + POSE_HEAD_SAVED_FLOATS, dtype=torch.float32, device=dev)      # one allocation for every output
        Rs, S, nll, saved = buf[:nj * 9].view(nj, 3, 3), buf[nj * 9:nj * 12].view(nj, 3), buf[nj * 12:nj * 13], buf[nj * 13:]
        a = PoseHeadArgs()
        _fill_head(a, poses, target_R, overreg, parents, params)
        a.Rs, a.S, a.nll, a.saved = Rs.data_ptr(), S.data_ptr(), nll.data_ptr(), saved.data_ptr()
        call("moss_pose_head_forward", dev, ctypes.byref(a))
        ctx.mark_non_differentiable(S)
        ctx.save_for_backward(poses, target_R, buf, *params)
        ctx.overreg, ctx.parents, ctx.sink = overreg, parents, sink
        return Rs, S, nll

    @staticmethod
    def backward(ctx, g_Rs, _g_S, g_nll):
        from ._lib import PoseHeadBackwardArgs, call, ptr
        poses, target_R, buf, *params = ctx.saved_tensors
        dev = poses.device
        nj = NUM_JOINTS
        sizes = [p.numel() for p in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)                 # every element is written by the kernel
        grads = [g.view(p.shape) for g, p in zip(flat.split(sizes), params)]
        if ctx.sink is not None:                                                         # (a sink replaces the parameter's scratch slice)
            grads = [_sunk(ctx.sink(i), g) for i, g in enumerate(grads)]
        g_Rs = None if g_Rs is None else g_Rs.float().contiguous()
        g_nll = None if g_nll is None else g_nll.float().contiguous()
        a = PoseHeadBackwardArgs()
        _fill_head(a, poses, target_R, ctx.overreg, ctx.parents, params)
        a.S, a.saved = buf[nj * 9:].data_ptr(), buf[nj * 13:].data_ptr()
        a.g_Rs, a.g_nll = ptr(g_Rs), ptr(g_nll)
        for i, g in enumerate(grads):
            a.grads[i] = g.data_ptr()
        call("moss_pose_head_backward", dev, ctypes.byref(a))
        return (None, None, None, None, None, *grads)


def _sunk(t, like):
    """A gradient sink's tensor in place of the scratch slice ``like`` (None: the slice stays)."""
    if t is None:
        return like
    if t.shape != like.shape or t.dtype != torch.float32 or t.device != like.device or not t.is_contiguous():
        raise ValueError(f"grad_sink returned a {t.dtype} tensor of shape {tuple(t.shape)} on {t.device} for a weight gradient of "
                         f"shape {tuple(like.shape)}: it must be contiguous float32 of the parameter's shape on its device")
    return t


def _fill_head(a, poses, target_R, overreg, parents, params):
    a.poses, a.target_R, a.overreg = poses.data_ptr(), target_R.data_ptr(), overreg
    for i, p in enumerate(params):
        a.params[i] = p.data_ptr()
    for i, p in enumerate(parents):
        a.parents[i] = p
    for j in range(NUM_JOINTS):
        a.fc_in[j] = params[6 + 2 * j].shape[1]


def _need_gpu(name, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{name} runs the HIP pose-head kernels: its tensors must be on a GPU "
                               "(autoregression_torch / matrix_fisher_nll are the torch form)")


def pose_head_fused(net, poses, target_R, overreg=1.005, parents=SMPL_PARENTS, grad_sink=None):
    """MOSS's ``pc.auto_regression(poses)`` followed by ``matrix_fisher_nll(...)``, one HIP kernel forward and one backward.

    ``net``: MOSS's ``Autoregression`` instance or anything with the same ``block_mlps`` / ``fc_pose`` parameters (float32, on the
    GPU); ``poses`` (1,72) or (72,); ``target_R`` (23,3,3) (any leading 1).  Returns ``{"Rs" (23,3,3), "pose_S" (23,3) the PROPER
    singular values, "nll" (23,), "target_R"}``.  Gradients flow from ``Rs`` and ``nll`` to the 52 parameters (``poses`` and
    ``target_R`` are data of the frame: no gradient is formed for them; ``pose_S`` carries none).  ``U`` and ``V`` are not returned:
    Rs is within 1e-5 of a rotation, so they are not unique, and only the loss reads them.

    ``grad_sink``: a callable ``param -> tensor or None`` (the contract of ``GradBucket.sink_for``), asked once per parameter in the
    backward.  Where it returns a tensor (contiguous float32, the parameter's shape) the backward kernel writes that parameter's
    gradient THERE and autograd receives that tensor; where it returns None the gradient stays a slice of the op's scratch tensor.  The
    kernel writes every element of every weight gradient, so a sink is OVERWRITTEN, not accumulated into: a sink must hand out each
    destination at most once per backward pass (``GradBucket.sink_for`` does)."""
    params = head_parameters(net)
    _need_gpu("pose_head_fused", poses, target_R, *params)
    dev = poses.device
    parents = tuple(int(p) for p in parents)
    if len(parents) != NUM_JOINTS + 1 or parents[0] != -1 or any(not 0 <= parents[i] < i for i in range(1, len(parents))):
        raise ValueError("pose_head_fused: parents must list 24 joints, -1 for the root and an earlier joint for every other")
    if poses.numel() != 72 or target_R.numel() != NUM_JOINTS * 9:
        raise ValueError("pose_head_fused: poses must hold 72 values and target_R 23 3x3 matrices")
    for name, p, shape in zip(PARAM_NAMES, params, _param_shapes(ancestor_lists(parents))):
        if tuple(p.shape) != shape or p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
            raise ValueError(f"pose_head_fused: {name} must be a contiguous float32 tensor of shape {shape} on {dev}, got "
                             f"{tuple(p.shape)} {p.dtype} on {p.device}")
    if poses.requires_grad or target_R.requires_grad:
        raise ValueError("pose_head_fused: poses and target_R are data of the frame (no gradient is formed for them); detach them")
    poses = poses.reshape(72).float().contiguous()
    tr = target_R.reshape(NUM_JOINTS, 3, 3).float().contiguous()
    sink = None if grad_sink is None else (lambda i: grad_sink(params[i]))
    Rs, S, nll = _PoseHead.apply(poses, tr, float(overreg), parents, sink, *params)
    return {"Rs": Rs, "pose_S": S, "nll": nll, "target_R": target_R}


class _MatrixFisherNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, target_R, overreg):
        from ._lib import call, ptr
        n, dev = int(F.shape[0]), F.device
        want = ctx.needs_input_grad[0]
        nll = torch.empty(n, dtype=torch.float32, device=dev)
        dF = torch.empty((n, 3, 3), dtype=torch.float32, device=dev) if want else None
        if n > 0:
            call("moss_matrix_fisher_nll", dev, n, F.data_ptr(), target_R.data_ptr(), overreg, nll.data_ptr(), ptr(dF))
        if want:
            ctx.save_for_backward(dF)
        return nll

    @staticmethod
    def backward(ctx, g):
        (dF,) = ctx.saved_tensors
        return g[:, None, None] * dF, None, None


def matrix_fisher_nll_fused(pred_F, target_R, overreg=1.005):
    """The matrix-Fisher NLL of ``target_R`` under general matrices ``pred_F`` (..., 3, 3): SVD, proper singular values, quadrature
    and -- when ``pred_F`` requires grad -- d nll / d F, in one HIP kernel (C ABI ``moss_matrix_fisher_nll``).  Returns (N,)."""
    _need_gpu("matrix_fisher_nll_fused", pred_F, target_R)
    if pred_F.shape[-2:] != (3, 3) or target_R.numel() != pred_F.numel():
        raise ValueError("matrix_fisher_nll_fused: pred_F and target_R must be (..., 3, 3) with the same number of matrices")
    if target_R.requires_grad:
        raise ValueError("matrix_fisher_nll_fused: target_R is data (no gradient is formed for it); detach it")
    F = pred_F.reshape(-1, 3, 3).float().contiguous()
    return _MatrixFisherNLL.apply(F, target_R.reshape(-1, 3, 3).to(F.device).float().contiguous(), float(overreg))
