"""The argument checks the SMPL / LBS ops share (``lbs.lbs_deform``, ``lbs.smpl_frame_fused``, ``posefit.posed_frame``, ``bounds``):
one tensor checker, one body-model check, one frame-parameter check.  Every refusal is a ``ValueError`` that begins with the op's name.
Imports without a GPU and without the built library."""
from __future__ import annotations

import torch

MAX_JOINTS = 64


def need(who, t, name, shape=None, dtype=torch.float32, numel=None, device=None):
    """``t`` if it is a contiguous tensor of ``dtype`` (and of ``shape``, of ``numel`` elements, on ``device``: those given)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a tensor")
    if t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{who}: {name} must be on {device}, got {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{who}: {name} must have {numel} elements, got {t.numel()}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    return t


def need_ids(who, vert_ids, device=None):
    if not isinstance(vert_ids, torch.Tensor) or vert_ids.dim() != 1:
        raise ValueError(f"{who}: vert_ids must be a (P,) tensor")
    return need(who, vert_ids, "vert_ids", dtype=torch.int64, device=device)


def no_grad(who, named, why):
    """Refuse a tensor of ``named`` (pairs or a dict of name -> tensor or None) that requires grad; ``why`` is the op's own clause."""
    for name, t in (named.items() if isinstance(named, dict) else named):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad, but {why}; detach it")


def need_gpu(who, dev, kernels, torch_form):
    if dev.type != "cuda":
        raise ValueError(f"{who} runs the HIP {kernels}: its tensors must be on a GPU ({torch_form})")


def body_arrays(who, body, why, kernels=None, torch_form=None, weights=None, check_weights=False):
    """``(V, J, parents, device)`` of an SMPL body model dict whose ``v_template`` (V,3), ``shapedirs`` (V,3,B), ``posedirs``
    (V,3,9(J-1)) and ``J_regressor`` (J,V) are float32, contiguous, on one GPU and require no grad (``why``: the op's clause of that
    refusal), with J = 1..64 and ``kintree_table[0]`` listing ``parent[j] < j``; ``parents`` are Python ints, joint 0's rewritten to -1
    (SMPL files store 2^32 - 1 there; it is not read).

    The blend weights, whose width is J: ``body['weights']``, held to the same standard only with ``check_weights`` (an op that hands
    them to its kernels), or the op's own argument ``weights`` (V,J), then named ``W`` and always checked.  ``kernels`` / ``torch_form``
    word the "must be on a GPU" refusal; without them it is left to the caller (:func:`need_gpu`), for an op whose remaining host checks
    come before it."""
    from .lbs import _parents
    own = weights is not None
    for key in ("v_template", "shapedirs", "posedirs", "J_regressor") + (() if own else ("weights",)) + ("kintree_table",):
        if not isinstance(body.get(key), torch.Tensor):
            raise ValueError(f"{who}: body['{key}'] must be a tensor")
    if own and (not isinstance(weights, torch.Tensor) or weights.dim() != 2):
        raise ValueError(f"{who}: W must be a (V, J) tensor")
    vt, sd, pd, jr = body["v_template"], body["shapedirs"], body["posedirs"], body["J_regressor"]
    w = weights if own else body["weights"]
    J = int(w.shape[-1])
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError(f"{who}: J = {J} joints; the kernels take 1..{MAX_JOINTS}")
    if vt.dim() != 2 or vt.shape[0] < 1:
        raise ValueError(f"{who}: v_template must be (V, 3) with V >= 1")
    V = int(vt.shape[0])
    if sd.dim() != 3:
        raise ValueError(f"{who}: shapedirs must be (V, 3, B)")
    dev = vt.device
    named = [("v_template", vt, (V, 3)), ("shapedirs", sd, (V, 3, sd.shape[2])), ("posedirs", pd, (V, 3, 9 * (J - 1))),
             ("J_regressor", jr, (J, V))] + ([("W" if own else "weights", w, (V, J))] if own or check_weights else [])
    no_grad(who, [(name, t) for name, t, _ in named], why)
    for name, t, shape in named:
        need(who, t, name, shape)
    if kernels is not None:
        need_gpu(who, dev, kernels, torch_form)
    for name, t, _ in named:
        if t.device != dev:
            raise ValueError(f"{who}: {name} must be on {dev}, got {t.device}")
    par = _parents(body, dev)[0]
    if len(par) != J or any(not 0 <= par[j] < j for j in range(1, J)):
        raise ValueError(f"{who}: kintree_table[0] must list J parents with 0 <= parent[j] < j for j >= 1")
    return V, J, [-1] + list(par[1:]), dev


def frame_params(who, params, keys, J, B, dev, name="params"):
    """``{key: the flattened tensor}`` of a frame's SMPL parameters ``params[key]`` for ``keys`` among ``poses`` (3J elements),
    ``shapes`` (at most ``B``, what ``shapedirs`` stores), ``R`` (9), ``Th`` (3): float32, contiguous, on ``dev``."""
    for key in keys:
        if not isinstance(params.get(key), torch.Tensor):
            raise ValueError(f"{who}: {name}['{key}'] must be a tensor")
    nb = int(params["shapes"].numel())
    if nb > B:
        raise ValueError(f"{who}: {nb} shape coefficients, but shapedirs stores {B}")
    count = {"poses": 3 * J, "shapes": nb, "R": 9, "Th": 3}
    return {key: need(who, params[key], f"{name}['{key}']", numel=count[key], device=dev).reshape(-1) for key in keys}
