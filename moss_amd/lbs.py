"""MOSS's per-frame linear blend skinning (``GaussianModel.coarse_deform_c2source``, scene/gaussian_model.py:820-923) on the device.

MOSS recomputes the per-Gaussian transforms on every render call (gaussian_renderer/__init__.py:60,72): nearest SMPL vertex, blend
weights (softmax over ``log(W + 1e-9) + lbs_weights`` with the pose refiner on), two blends of the 24 joint transforms, a batched
``torch.inverse`` -- which synchronises with the host -- and a chain of batched 3x3 products, forward and backward.  Here:

* :func:`lbs_deform` -- the per-Gaussian part, one HIP kernel each way (C ABI ``moss_lbs_deform_forward`` / ``_backward``,
  moss_amd/csrc/lbs.hip): weights, both blends, the 3x3 inverse (adjugate), ``T``, ``t`` and the posed positions ``p``.  Gradients go
  to the LBS offsets, ``A_obs`` (a deterministic reduction over the Gaussians), the gathered offsets ``d`` and the positions ``x``.
* :func:`smpl_joint_transforms`, :func:`vertex_offsets` -- the per-frame, per-subject part in torch (24 joints, two GEMVs): small in
  bytes, about 320 launches per training step; differentiable, no host synchronisation.
* :func:`smpl_frame_fused` -- the same per-frame part as a fused HIP op (C ABI ``moss_smpl_frame_forward`` / ``_backward``,
  moss_amd/csrc/smpl_frame.hip): both Rodrigues, both chains, the offset table in one pass over ``posedirs`` and its gather, two
  launches forward and three backward.  The gradient goes to ``correct_Rs``.
* :func:`coarse_deform_c2source` -- the drop-in: same arguments, same 5-tuple as the reference.
* :func:`deform_torch` -- the same per-Gaussian math in plain torch (any dtype or device): the float64 yardstick of the tests and the
  float32 stand-in for MOSS's chain in scripts/lbs_times.py.  It is not a fallback; :func:`lbs_deform` has no CPU path.
* :func:`synthetic_body_model` -- a seeded SMPL-shaped body model for tests, the fixture generator and the timing script.

Everything here imports without a GPU.
"""
from __future__ import annotations

import ctypes
import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.weak import WeakIdKeyDictionary

from ._checks import MAX_JOINTS, body_arrays, frame_params, need, need_gpu, need_ids, no_grad
from ._lib import (LbsBackwardArgs, LbsBackwardFrameArgs, LbsForwardArgs, SMPL_FRAME_SAVED_FLOATS_PER_JOINT, SmplFrameArgs,
                   SmplFrameBackwardArgs, SmplFrameBackwardPoseArgs, call, lib, ptr)

__all__ = ["lbs_deform", "smpl_joint_transforms", "vertex_offsets", "smpl_frame_fused", "coarse_deform_c2source", "deform_torch",
           "synthetic_body_model", "batch_rodrigues", "MAX_JOINTS", "SMPL_PARENTS"]

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def _c32(g):
    return None if g is None else g.float().contiguous()


# ---- the per-Gaussian op -------------------------------------------------------------------------------------------------------

def _fill_inputs(a, ids, W, L, A_big, A_obs, d, R, Th, x):
    a.P, a.J, a.V = int(ids.shape[0]), int(W.shape[1]), int(W.shape[0])
    a.vert_ids, a.weights, a.lbs_offsets = ids.data_ptr(), W.data_ptr(), ptr(L)
    a.A_big, a.A_obs, a.d, a.R, a.Th, a.x = A_big.data_ptr(), A_obs.data_ptr(), d.data_ptr(), R.data_ptr(), Th.data_ptr(), ptr(x)


def _launch_lbs_forward(ids, W, L, A_big, A_obs, d, R, Th, x, want_weights):
    """``moss_lbs_deform_forward`` (no launch at P = 0): ``(T, t, p or None without x, w or None)``."""
    P, J = int(ids.shape[0]), int(W.shape[1])
    dev = W.device
    T = torch.empty((P, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((P, 3), dtype=torch.float32, device=dev)
    p = torch.empty((P, 3), dtype=torch.float32, device=dev) if x is not None else None
    w = torch.empty((P, J), dtype=torch.float32, device=dev) if want_weights else None
    if P > 0:
        a = LbsForwardArgs()
        _fill_inputs(a, ids, W, L, A_big, A_obs, d, R, Th, x)
        a.T, a.t, a.p, a.w = T.data_ptr(), t.data_ptr(), ptr(p), ptr(w)
        call("moss_lbs_deform_forward", dev, ctypes.byref(a))
    return T, t, p, w


def _launch_lbs_backward(inputs, gT, gt, gp, want):
    """The gradients named in ``want`` (``g_L``, ``g_A_obs``, ``g_d``, ``g_x``, ``g_R``, ``g_Th``: fields of the args block) of the
    forward's ``inputs``, as a dict.  With ``g_R`` among them ``moss_lbs_deform_backward_frame`` (the plain block plus ``g_R``,
    ``g_Th``; launched whatever P is), else ``moss_lbs_deform_backward``: no launch when nothing is wanted or P = 0, and only then is
    ``g_A_obs`` zeros."""
    ids, W, x = inputs[0], inputs[1], inputs[8]
    P, J = int(ids.shape[0]), int(W.shape[1])
    dev = W.device
    frame = "g_R" in want
    launch = frame or (P > 0 and bool(want))
    shapes = {"g_L": (P, J), "g_A_obs": (J, 4, 4), "g_d": (P, 3), "g_x": (P, 3), "g_R": (3, 3), "g_Th": (3,)}
    g = {k: (torch.empty if launch or k != "g_A_obs" else torch.zeros)(shapes[k], dtype=torch.float32, device=dev) for k in want}
    if launch:
        a = (LbsBackwardFrameArgs if frame else LbsBackwardArgs)()
        _fill_inputs(a, *inputs)
        gT, gt, gp = _c32(gT), _c32(gt), (None if x is None else _c32(gp))
        a.g_T, a.g_t, a.g_p = ptr(gT), ptr(gt), ptr(gp)
        for k, t in g.items():
            setattr(a, k, t.data_ptr())
        if "g_A_obs" in g:
            nbytes = int((lib().moss_lbs_frame_workspace_bytes if frame else lib().moss_lbs_workspace_bytes)(P, J))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a.workspace, a.workspace_bytes = (ws.data_ptr() if nbytes else None), nbytes
        call("moss_lbs_deform_backward_frame" if frame else "moss_lbs_deform_backward", dev, ctypes.byref(a))
    return g


class _LbsDeform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, W, L, A_big, A_obs, d, R, Th, x, want_weights):
        T, t, p, w = _launch_lbs_forward(ids, W, L, A_big, A_obs, d, R, Th, x, want_weights)
        if w is not None:
            ctx.mark_non_differentiable(w)
        ctx.save_for_backward(ids, W, L, A_big, A_obs, d, R, Th, x)
        ctx.has_L, ctx.has_x = L is not None, x is not None
        return T, t, p, w

    @staticmethod
    def backward(ctx, gT, gt, gp, _gw):
        inputs = list(ctx.saved_tensors)
        inputs[2] = inputs[2] if ctx.has_L else None
        inputs[8] = inputs[8] if ctx.has_x else None
        wanted = ctx.needs_input_grad
        g = _launch_lbs_backward(inputs, gT, gt, gp, [k for k, yes in (("g_L", wanted[2] and ctx.has_L), ("g_A_obs", wanted[4]),
                                                                       ("g_d", wanted[5]), ("g_x", wanted[8] and ctx.has_x)) if yes])
        return None, None, g.get("g_L"), None, g.get("g_A_obs"), g.get("g_d"), None, None, g.get("g_x"), None


def lbs_deform(vert_ids, W, lbs_offsets, A_big, A_obs, d, R, Th, x=None, want_weights=False):
    """Per-Gaussian LBS of one frame on the device (C ABI ``moss_lbs_deform_forward`` / ``_backward``; formulas in
    include/moss_raster.h).  Returns ``(T (P,3,3), t (P,3), p (P,3) or None, w (P,J) or None)``: MOSS's ``transforms``,
    ``translation``, ``world_src_pts`` (needs ``x``) and ``bweights`` (with ``want_weights``; not differentiable).

    ``vert_ids`` (P,) int64; ``W`` (V,J); ``lbs_offsets`` (P,J) or None; ``A_big``, ``A_obs`` (J,4,4); ``d`` (P,3) the per-vertex
    offsets already gathered at ``vert_ids``; ``R`` (3,3); ``Th`` (3,); ``x`` (P,3) or None.  All float32, contiguous, on one GPU;
    J = 1..64.  Gradients flow to ``lbs_offsets``, ``A_obs``, ``d`` and ``x``; ``A_big``, ``R``, ``Th`` and ``W`` are constants of
    MOSS's step and must not require grad (ValueError).  Ids outside [0, V) give NaN rows."""
    if not isinstance(W, torch.Tensor) or W.dim() != 2:
        raise ValueError("lbs_deform: W must be a (V, J) tensor")
    dev = W.device
    need_gpu("lbs_deform", dev, "LBS kernels", "deform_torch is the torch form")
    V, J = int(W.shape[0]), int(W.shape[1])
    if not 1 <= J <= MAX_JOINTS:
        raise ValueError(f"lbs_deform: J = {J} joints; the kernels take 1..{MAX_JOINTS}")
    if V < 1:
        raise ValueError("lbs_deform: W has no vertices")
    P = int(need_ids("lbs_deform", vert_ids, dev).shape[0])
    for name, t, shape in (("W", W, (V, J)), ("lbs_offsets", lbs_offsets, (P, J)), ("A_big", A_big, (J, 4, 4)), ("A_obs", A_obs, (J, 4, 4)),
                           ("d", d, (P, 3)), ("R", R, (3, 3)), ("Th", Th, (3,)), ("x", x, (P, 3))):
        if t is not None or name not in ("lbs_offsets", "x"):
            need("lbs_deform", t, name, shape, device=dev)
    no_grad("lbs_deform", (("W", W), ("A_big", A_big), ("R", R), ("Th", Th)),
            "it is a constant of the deformation (no gradient is formed for it)")
    return _LbsDeform.apply(vert_ids, W, lbs_offsets, A_big, A_obs, d, R, Th, x, bool(want_weights))


def deform_torch(vert_ids, W, lbs_offsets, A_big, A_obs, d, R, Th, x=None):
    """The math of :func:`lbs_deform` in plain torch, in the inputs' dtype and on their device: ``(T, t, p or None, w)``.
    The float64 yardstick of the tests and the float32 stand-in for MOSS's torch chain (it inverts with ``torch.inverse`` as MOSS
    does, which synchronises with the host on a GPU)."""
    w = W[vert_ids]
    if lbs_offsets is not None:
        w = F.softmax(torch.log(w + 1e-9) + lbs_offsets, dim=-1)
    J = W.shape[1]
    B = (w @ A_big.reshape(J, 16)).reshape(-1, 4, 4)
    O = (w @ A_obs.reshape(J, 16)).reshape(-1, 4, 4)
    Q = torch.inverse(B[:, :3, :3])
    M = R @ O[:, :3, :3]
    T = M @ Q
    u = d - (Q @ B[:, :3, 3:]).squeeze(-1)
    t = (M @ u[..., None]).squeeze(-1) + O[:, :3, 3] @ R.T + Th
    p = None if x is None else (T @ x[..., None]).squeeze(-1) + t
    return T, t, p, w


# ---- the per-frame part in torch ------------------------------------------------------------------------------------------------

def batch_rodrigues(rot_vecs):
    """(N,3) axis-angle -> (N,3,3) rotations, the formula of the reference's two Rodrigues helpers (gaussian_model.py:945-963,1033-1061):
    angle = |r + 1e-8|, R = I + sin K + (1 - cos) K^2."""
    n = rot_vecs.shape[0]
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    rx, ry, rz = torch.split(rot_vecs / angle, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(n, 3, 3)
    cos = torch.cos(angle)[:, None]
    sin = torch.sin(angle)[:, None]
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)[None]
    return eye + sin * K + (1 - cos) * torch.bmm(K, K)


_PARENTS = WeakIdKeyDictionary()


def _parents(body, device):
    """(the parent list as Python ints, the parents of joints 1.. as an index tensor on ``device``), made once per kintree table and
    device: a table on the GPU costs one host read and the index one copy, at the first (eager) call -- never inside a capture."""
    kt = body["kintree_table"]
    entry = _PARENTS.get(kt)
    if entry is None:
        entry = _PARENTS[kt] = ([int(v) for v in kt[0].tolist()], {})
    par, idx = entry
    if device not in idx:
        idx[device] = torch.tensor(par[1:], dtype=torch.long, device=device)
    return par, idx[device]


def _betas(params, like):
    return params["shapes"].reshape(1, -1).to(like)


def smpl_joint_transforms(body, params, rot_mats=None):
    """The SMPL kinematic chain of one frame: ``(A (1,J,4,4), R, Th)`` -- what the reference's ``get_transform_params_torch``
    (gaussian_model.py:965-1031) returns but the joints.  Shaped template -> ``J_regressor`` joints -> relative joints -> the parent
    chain of 4x4 products -> the rest joints subtracted.  ``rot_mats`` (1,J,3,3) or (J,3,3), default the Rodrigues of
    ``params['poses']``.  Differentiable (through ``rot_mats`` and the shapes), no host synchronisation: capturable."""
    W = body["weights"]
    J = W.shape[-1]
    vt = body["v_template"]
    betas = _betas(params, vt)
    nb = betas.shape[-1]
    v_shaped = vt + (body["shapedirs"][..., :nb] * betas[0]).sum(-1)
    joints = body["J_regressor"] @ v_shaped                                   # (J,3)
    if rot_mats is None:
        rot_mats = batch_rodrigues(params["poses"].reshape(-1, 3).to(vt))
    rot_mats = rot_mats.reshape(J, 3, 3)
    par, idx = _parents(body, joints.device)
    rel = torch.cat([joints[:1], joints[1:] - joints[idx]], 0)
    bottom = torch.zeros((J, 1, 4), dtype=vt.dtype, device=vt.device)
    bottom[..., 3] = 1
    local = torch.cat([torch.cat([rot_mats, rel[..., None]], -1), bottom], -2)   # (J,4,4)
    chain = [local[0]]
    for i in range(1, J):
        chain.append(chain[par[i]] @ local[i])
    G = torch.stack(chain, 0)
    rest = (G[:, :3, :3] @ joints[..., None]).squeeze(-1)
    A = torch.cat([G[:, :, :3], torch.cat([G[:, :3, 3] - rest, G[:, 3:, 3]], -1)[..., None]], -1)
    return A[None], params["R"], params["Th"]


def _pose_offsets(body, rot_mats):
    J = rot_mats.shape[-3]
    pd = body["posedirs"]
    V = pd.shape[0]
    eye = torch.eye(3, dtype=rot_mats.dtype, device=rot_mats.device)
    feat = (rot_mats.reshape(J, 3, 3)[1:] - eye).reshape(-1)
    return (pd.reshape(V * 3, -1) @ feat).reshape(V, 3)


def vertex_offsets(body, params, t_params, rot_mats):
    """The per-vertex offset table ``D = shape_off - pose_off_big + pose_off_obs`` (V,3) of the reference's mean-shape branch
    (gaussian_model.py:852-899): the pose blend shapes of the big pose (``t_params['poses']``) and of the frame (``rot_mats``, the
    refined rotations when the pose refiner runs), and the shape blend shapes of ``params['shapes']``, one GEMV each.

    MOSS gathers it per Gaussian with ``torch.gather`` at the nearest vertex; :func:`coarse_deform_c2source` does the same with
    ``D[vert_ids]``, so the backward of that one gather (an index accumulation into (V,3)) is torch's, not this module's kernels'."""
    vt = body["v_template"]
    big = batch_rodrigues(t_params["poses"].reshape(-1, 3).to(vt))
    betas = _betas(params, vt)
    shape_off = (body["shapedirs"][..., :betas.shape[-1]] * betas[0]).sum(-1)
    return shape_off - _pose_offsets(body, big) + _pose_offsets(body, rot_mats)


# ---- the per-frame part as a fused op -------------------------------------------------------------------------------------------

def _launch_smpl_frame_forward(cR, par, vt, sd, pd, jr, poses_big, shapes_big, poses, shapes, ids, want_saved):
    """``moss_smpl_frame_forward``: ``(A_big, A_obs, d, rot_mats, saved or None)``."""
    V, J, P = int(vt.shape[0]), int(jr.shape[0]), int(ids.shape[0])
    dev = vt.device
    f32 = dict(dtype=torch.float32, device=dev)
    A_big, A_obs = torch.empty((J, 4, 4), **f32), torch.empty((J, 4, 4), **f32)
    d, rot = torch.empty((P, 3), **f32), torch.empty((J, 3, 3), **f32)
    saved = torch.empty(SMPL_FRAME_SAVED_FLOATS_PER_JOINT * J, **f32) if want_saved else None
    nbytes = int(lib().moss_smpl_frame_workspace_bytes(max(P, 1), V, J))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = SmplFrameArgs()
    a.P, a.V, a.J = P, V, J
    a.num_betas_big, a.num_betas, a.shapedirs_stride = int(shapes_big.shape[0]), int(shapes.shape[0]), int(sd.shape[2])
    a.parents[:J] = par
    a.v_template, a.shapedirs, a.posedirs, a.J_regressor = vt.data_ptr(), sd.data_ptr(), pd.data_ptr(), jr.data_ptr()
    a.poses_big, a.shapes_big, a.poses, a.shapes = poses_big.data_ptr(), shapes_big.data_ptr(), poses.data_ptr(), shapes.data_ptr()
    a.correct_Rs, a.vert_ids = ptr(cR), ids.data_ptr()
    a.A_big, a.A_obs, a.d, a.rot_mats, a.saved = A_big.data_ptr(), A_obs.data_ptr(), d.data_ptr(), rot.data_ptr(), ptr(saved)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    call("moss_smpl_frame_forward", dev, ctypes.byref(a))
    return A_big, A_obs, d, rot, saved


def _launch_smpl_frame_backward(par, V, pd, ids, saved, gA_obs, gd, poses=None, cR=None):
    """Without ``poses`` ``moss_smpl_frame_backward`` (no launch at J = 1): ``g_correct_Rs`` (J-1,3,3).  With ``poses`` (and the
    forward's ``cR``) ``moss_smpl_frame_backward_pose``, the same block plus ``poses``, ``correct_Rs``, ``g_poses``: ``g_poses`` (3J)."""
    J, P = len(par), int(ids.shape[0])
    dev = pd.device
    pose = poses is not None
    g = torch.empty(3 * J if pose else (J - 1, 3, 3), dtype=torch.float32, device=dev)
    if pose or J > 1:
        a = (SmplFrameBackwardPoseArgs if pose else SmplFrameBackwardArgs)()
        a.P, a.V, a.J = P, V, J
        a.parents[:J] = par
        a.posedirs, a.vert_ids, a.saved = pd.data_ptr(), ids.data_ptr(), saved.data_ptr()
        gA_obs, gd = _c32(gA_obs), (None if P == 0 else _c32(gd))
        a.g_A_obs, a.g_d = ptr(gA_obs), ptr(gd)
        if pose:
            a.poses, a.correct_Rs, a.g_poses = poses.data_ptr(), ptr(cR), g.data_ptr()
        else:
            a.g_correct_Rs = g.data_ptr()
        if pose or gd is not None:
            nbytes = int(lib().moss_smpl_frame_workspace_bytes(max(P, 1), V, J))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        call("moss_smpl_frame_backward_pose" if pose else "moss_smpl_frame_backward", dev, ctypes.byref(a))
    return g


class _SmplFrame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cR, par, vt, sd, pd, jr, poses_big, shapes_big, poses, shapes, ids):
        A_big, A_obs, d, rot, saved = _launch_smpl_frame_forward(cR, par, vt, sd, pd, jr, poses_big, shapes_big, poses, shapes, ids,
                                                                 want_saved=cR is not None)
        ctx.mark_non_differentiable(A_big, rot)
        ctx.set_materialize_grads(False)                        # (no zero-fill launches for the cotangents nobody formed)
        if cR is not None:
            ctx.save_for_backward(pd, ids, saved)
        ctx.par, ctx.V = par, int(vt.shape[0])
        return A_big, A_obs, d, rot

    @staticmethod
    def backward(ctx, _gA_big, gA_obs, gd, _grot):
        if not ctx.needs_input_grad[0]:
            return (None,) * 11
        pd, ids, saved = ctx.saved_tensors
        return (_launch_smpl_frame_backward(ctx.par, ctx.V, pd, ids, saved, gA_obs, gd),) + (None,) * 10


def smpl_frame_fused(body, params, t_params, vert_ids, correct_Rs=None):
    """The per-frame, per-subject part of ``coarse_deform_c2source`` as one fused op on the device (C ABI ``moss_smpl_frame_forward`` /
    ``_backward``; formulas in include/moss_raster.h): ``(A_big (J,4,4), A_obs (J,4,4), d (P,3), rot_mats (J,3,3))`` -- what
    :func:`smpl_joint_transforms` of ``t_params`` and of ``params`` (with ``rot[1:] @ correct_Rs``), :func:`vertex_offsets` gathered at
    ``vert_ids``, and the frame's refined rotations give, in two launches.  ``D`` is formed in one pass over ``posedirs``
    (``P f_obs - P f_big = P (f_obs - f_big)``) and every sum in float64, so the rounding differs from the torch form's within the
    float32 bar of the tests.

    ``body``: ``v_template`` (V,3), ``shapedirs`` (V,3,B), ``posedirs`` (V,3,9(J-1)), ``J_regressor`` (J,V), ``weights`` (V,J) (its
    width is J), ``kintree_table`` (2,J) with ``parent[j] < j`` (read on the host once per table, never inside a capture).
    ``params`` / ``t_params``: ``poses`` (3J elements), ``shapes`` (at most B elements).  ``vert_ids`` (P,) int64; ``correct_Rs``
    (J-1,3,3) or None.  All float32, contiguous, on one GPU; J = 1..64.  The gradient flows to ``correct_Rs`` (from ``A_obs`` and
    ``d``); ``A_big`` and ``rot_mats`` come out detached, and ``poses``, ``shapes`` and the body model are data: one that requires
    grad raises ValueError.  Ids outside [0, V) give NaN rows of ``d``.  There is no CPU path."""
    who, why = "smpl_frame_fused", "it is data of the deformation (no gradient is formed for it)"
    # (the "must be on a GPU" refusal comes after the frame's own checks: CPU tensors with another fault are told that fault)
    _, J, par, dev = body_arrays(who, body, why)
    B = int(body["shapedirs"].shape[2])
    big = frame_params(who, t_params, ("poses", "shapes"), J, B, dev, name="t_params")
    frame = frame_params(who, params, ("poses", "shapes"), J, B, dev)
    no_grad(who, [(f"{name}['{k}']", t) for name, p in (("params", frame), ("t_params", big)) for k, t in p.items()], why)
    need_ids(who, vert_ids, dev)
    if correct_Rs is not None:
        need(who, correct_Rs, "correct_Rs", (J - 1, 3, 3), device=dev)
    need_gpu(who, dev, "per-frame kernels", "smpl_joint_transforms and vertex_offsets are the torch form")
    return _SmplFrame.apply(correct_Rs, par, body["v_template"], body["shapedirs"], body["posedirs"], body["J_regressor"], big["poses"],
                            big["shapes"], frame["poses"], frame["shapes"], vert_ids)


def coarse_deform_c2source(model, query_pts, params, t_params, t_vertices, lbs_weights=None, correct_Rs=None, return_transl=False,
                           fused_frame=False):
    """Drop-in for ``GaussianModel.coarse_deform_c2source`` (scene/gaussian_model.py:820-923): same arguments, same
    ``(smpl_src_pts, world_src_pts, bweights, transforms, translation)`` of shapes (1,P,3), (1,P,3), (1,P,J), (1,P,3,3), (1,P,3) --
    ``translation`` only with ``return_transl``, else None.  ``model`` supplies ``SMPL_NEUTRAL`` (the body model, on the GPU) and
    ``knn`` (``moss_amd.knn_cuda.KNN(k=1, transpose_mode=True)``), as MOSS's ``GaussianModel`` does; a model with a ``template_index``
    (a ``knn_cuda.TemplateIndex`` over ``t_vertices``, an addition) is asked through it instead: the same ids.  The per-Gaussian work is
    :func:`lbs_deform`; the kinematic chain and the blend shapes are torch, or with ``fused_frame`` (an addition, default off) the
    fused op :func:`smpl_frame_fused`.  ``bweights`` carries no gradient (MOSS only accumulates it for densification).  Batch size 1,
    as MOSS renders."""
    if query_pts.dim() != 3 or query_pts.shape[0] != 1:
        raise ValueError("coarse_deform_c2source: query_pts must be (1, P, 3)")
    body = model.SMPL_NEUTRAL
    W = body["weights"]
    J = W.shape[-1]
    P = query_pts.shape[1]
    index = getattr(model, "template_index", None)
    if index is not None:
        # (an addition, opt-in: a knn_cuda.TemplateIndex built once over t_vertices -- the same ids, one launch, no grid build per call)
        if index.V != t_vertices.shape[-2]:
            raise ValueError(f"coarse_deform_c2source: model.template_index holds {index.V} vertices, t_vertices has {t_vertices.shape[-2]}")
        ids = index.query(query_pts[0])
    else:
        _, vert_ids = model.knn(t_vertices.float(), query_pts.float())
        ids = vert_ids.reshape(P)
    if fused_frame:
        c32 = lambda t: t.float().contiguous()                                        # noqa: E731
        A_big, A_obs, d, _ = smpl_frame_fused(
            body, {"poses": c32(params["poses"]), "shapes": c32(params["shapes"])},
            {"poses": c32(t_params["poses"]), "shapes": c32(t_params["shapes"])}, ids.contiguous(),
            correct_Rs=None if correct_Rs is None else c32(correct_Rs.reshape(J - 1, 3, 3)))
        return _deform_frame(query_pts, ids, W, lbs_weights, A_big, A_obs, d, params["R"], params["Th"], return_transl)
    A_big, _, _ = smpl_joint_transforms(body, t_params)
    rot_mats = batch_rodrigues(params["poses"].reshape(-1, 3).to(W)).reshape(J, 3, 3)
    if correct_Rs is not None:
        rot_mats = torch.cat([rot_mats[:1], rot_mats[1:] @ correct_Rs.reshape(J - 1, 3, 3)], 0)
    A_obs, R, Th = smpl_joint_transforms(body, params, rot_mats=rot_mats)
    D = vertex_offsets(body, params, t_params, rot_mats)
    d = D[ids]
    return _deform_frame(query_pts, ids, W, lbs_weights, A_big[0].detach(), A_obs[0], d, R, Th, return_transl)


def _deform_frame(query_pts, ids, W, lbs_weights, A_big, A_obs, d, R, Th, return_transl):
    """The per-Gaussian half of :func:`coarse_deform_c2source`, from the frame's ``A_big``, ``A_obs`` (J,4,4) and ``d`` (P,3)."""
    P, J = ids.shape[0], W.shape[-1]
    L = None if lbs_weights is None else lbs_weights.reshape(P, J).float().contiguous()
    R = R.reshape(3, 3).float().contiguous()
    Th = Th.reshape(3).float().contiguous()
    T, t, p, w = lbs_deform(ids.contiguous(), W.contiguous(), L, A_big.contiguous(), A_obs.contiguous(),
                            d.contiguous(), R, Th, x=query_pts[0].float().contiguous(), want_weights=True)
    smpl_src = (p - Th) @ R                                    # R^T (p - Th): the reference's smpl_src_pts
    return smpl_src[None], p[None], w[None], T[None], (t[None] if return_transl else None)


# ---- a synthetic body model -----------------------------------------------------------------------------------------------------

def synthetic_body_model(V, J=24, seed=0, num_betas=10, device="cpu"):
    """A seeded SMPL-shaped body model (numpy PCG64): the dict keys of MOSS's ``SMPL_NEUTRAL`` -- ``v_template`` (V,3),
    ``shapedirs`` (V,3,num_betas), ``posedirs`` (V,3,9(J-1)), ``J_regressor`` (J,V), ``kintree_table`` (2,J) int64, ``weights`` (V,J)
    -- with SMPL's 24-joint parent list (a seeded tree past 24), sparse normalised weights (a vertex's home joint, its parent and
    one more), a regressor that averages each joint's vertices, and small blend shapes.  Float32 tensors on ``device``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    par = list(SMPL_PARENTS[:min(J, 24)]) + [int(rng.integers(0, j)) for j in range(24, J)]
    jpos = np.zeros((J, 3))
    for j in range(1, J):
        step = rng.normal(size=3)
        jpos[j] = jpos[par[j]] + 0.2 * step / np.linalg.norm(step)
    home = np.concatenate([np.arange(J), rng.integers(0, J, size=max(V - J, 0))])[:V]
    v_template = jpos[home] + 0.05 * rng.normal(size=(V, 3))
    weights = np.zeros((V, J))
    for v in range(V):
        j = home[v]
        weights[v, j] = 1.0 + rng.random()
        if j > 0:
            weights[v, par[j]] += rng.random()
        weights[v, int(rng.integers(0, J))] += 0.3 * rng.random()
    weights /= weights.sum(1, keepdims=True)
    J_regressor = np.zeros((J, V))
    for j in range(J):
        mine = np.nonzero(home == j)[0]
        J_regressor[j, mine] = 1.0 / max(len(mine), 1)
    shapedirs = 0.01 * rng.normal(size=(V, 3, num_betas))
    posedirs = 0.005 * rng.normal(size=(V, 3, 9 * (J - 1)))
    kintree = np.stack([np.array(par), np.arange(J)]).astype(np.int64)
    f32 = dict(dtype=torch.float32, device=device)
    return {"v_template": torch.tensor(v_template, **f32), "shapedirs": torch.tensor(shapedirs, **f32),
            "posedirs": torch.tensor(posedirs, **f32), "J_regressor": torch.tensor(J_regressor, **f32),
            "kintree_table": torch.tensor(kintree, dtype=torch.int64), "weights": torch.tensor(weights, **f32)}


def synthetic_frame(seed, J=24, big_pose=False, device="cpu"):
    """Seeded SMPL parameters of one frame: ``poses`` (1,3J) (MOSS's big pose: legs spread 45 / 30 degrees), ``shapes`` (1,10),
    ``R`` (3,3) a rotation, ``Th`` (1,3)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f32 = dict(dtype=torch.float32, device=device)
    if big_pose:
        poses = np.zeros((1, 3 * J))
        poses[0, 5], poses[0, 8], poses[0, 23], poses[0, 26] = np.pi / 4, -np.pi / 4, -np.pi / 6, np.pi / 6
        return {"poses": torch.tensor(poses, **f32), "shapes": torch.zeros((1, 10), **f32), "R": torch.eye(3, **f32),
                "Th": torch.zeros((1, 3), **f32)}
    poses = 0.3 * rng.normal(size=(1, 3 * J))
    axis = rng.normal(size=3)
    Rm = batch_rodrigues(torch.tensor(axis / np.linalg.norm(axis) * rng.uniform(0.3, 2.5))[None])[0].numpy()
    return {"poses": torch.tensor(poses, **f32), "shapes": torch.tensor(0.5 * rng.normal(size=(1, 10)), **f32),
            "R": torch.tensor(Rm, **f32), "Th": torch.tensor(rng.normal(size=(1, 3)), **f32)}
