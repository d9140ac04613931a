"""Fitting a frame's SMPL pose to keypoints: the posed vertices as a differentiable HIP op and a keypoint loss on top of them.

The photometric term of :class:`moss_amd.posefit.PoseFitter` converges only from a pose that already overlaps the person in the image.
What new footage comes with is a 2D detector's keypoints, or triangulated / mocap 3D points; keypoints of any convention (OpenPose,
COCO, H36M, markers glued to vertices) are a linear regressor over the posed vertices.

* :func:`posed_vertices_fn` -- ``world_vertex`` (V,3) of one frame as an ``autograd.Function``: forward = ``moss_smpl_vertices`` (the
  bits of ``bounds.posed_vertices``), backward = ``moss_smpl_vertices_backward`` (include/moss_raster.h; csrc/frame_bounds.hip): four
  launches, nothing saved by the forward.  Gradients go to ``params['poses']``, ``params['R']`` and ``params['Th']`` and to nothing else.
* :func:`keypoint_loss` -- ``moss_keypoint_loss`` (csrc/keypoints.hip): the loss of :class:`KeypointTargets` and its gradient to the
  vertices in one call of three launches; the backward is one multiplication.
* :func:`keypoint_loss_torch` / :func:`project_torch` -- the same contract in torch ops, in the inputs' dtype and on any device: with
  ``bounds.posed_vertices_torch`` the float64 yardstick of the tests and the float32 stand-in of scripts/keypoint_fit_times.py.  It
  is not a fallback; the two ops above have no CPU path.

Float64 sums in a fixed order, no atomics, bitwise reproducible, capturable.  Everything here imports without a GPU.
"""
from __future__ import annotations

import ctypes

import torch

from ._checks import body_arrays, frame_params, need, need_gpu, no_grad

__all__ = ["posed_vertices_fn", "keypoint_loss", "keypoint_loss_torch", "project_torch", "KeypointTargets", "KEYPOINTS_MAX"]

KEYPOINTS_MAX = 128                                              # MOSS_KEYPOINTS_MAX
_WHY = "it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only)"
_WHY_TARGET = "the targets are data of the loss (its gradient goes to world_vertex only)"


# ---- the posed vertices ---------------------------------------------------------------------------------------------------------------

class _PosedVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, R, Th, shapes, body, V, J, par):
        from ._lib import lib
        from .bounds import _launch_vertices
        dev = poses.device
        world_vertex = torch.empty((V, 3), dtype=torch.float32, device=dev)
        scratch = torch.zeros(7, dtype=torch.float32, device=dev)         # (the entry's world_bound, not returned, and a zero pad)
        ws = torch.empty(int(lib().moss_smpl_vertices_workspace_bytes(V, J)), dtype=torch.uint8, device=dev)
        _launch_vertices(body, V, J, par, poses, shapes, R, Th, scratch[6:], world_vertex, scratch[:6], None, ws)
        ctx.save_for_backward(poses, R, Th, shapes)
        ctx.body, ctx.V, ctx.J, ctx.par = body, V, J, par
        return world_vertex

    @staticmethod
    def backward(ctx, g):
        from ._lib import SmplVerticesBackwardArgs, call, lib
        poses, R, Th, shapes = ctx.saved_tensors
        body, V, J = ctx.body, ctx.V, ctx.J
        dev = poses.device
        g = g.contiguous()
        g_poses, g_R, g_Th = (torch.empty(n, dtype=torch.float32, device=dev) for n in (3 * J, 9, 3))
        ws = torch.empty(int(lib().moss_smpl_vertices_backward_workspace_bytes(V, J)), dtype=torch.uint8, device=dev)
        a = SmplVerticesBackwardArgs()
        a.V, a.J, a.num_betas, a.shapedirs_stride = V, J, int(shapes.numel()), int(body["shapedirs"].shape[2])
        a.parents[:J] = ctx.par
        a.v_template, a.shapedirs, a.posedirs = body["v_template"].data_ptr(), body["shapedirs"].data_ptr(), body["posedirs"].data_ptr()
        a.J_regressor, a.weights = body["J_regressor"].data_ptr(), body["weights"].data_ptr()
        a.poses, a.shapes, a.R, a.Th = poses.data_ptr(), shapes.data_ptr(), R.data_ptr(), Th.data_ptr()
        a.g_world_vertex = g.data_ptr()
        a.g_poses, a.g_R, a.g_Th = g_poses.data_ptr(), g_R.data_ptr(), g_Th.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        call("moss_smpl_vertices_backward", dev, ctypes.byref(a))
        return g_poses, g_R, g_Th, None, None, None, None, None


def posed_vertices_fn(body, params):
    """``world_vertex`` (V,3) of one frame on the device, with gradients to ``params['poses']``, ``params['R']`` and ``params['Th']``
    (C ABI ``moss_smpl_vertices`` forward: the bits of ``bounds.posed_vertices``; ``moss_smpl_vertices_backward`` backward, four
    launches; formulas in include/moss_raster.h).

    ``body``: ``v_template`` (V,3), ``shapedirs`` (V,3,B), ``posedirs`` (V,3,9(J-1)), ``J_regressor`` (J,V), ``weights`` (V,J),
    ``kintree_table`` (2,J); ``params``: ``poses`` (3J elements), ``shapes`` (at most B), ``R`` (3,3), ``Th`` (3 elements).  All
    float32, contiguous, on one GPU; J = 1..64.  ``shapes`` and the body model are data: one that requires grad raises ``ValueError``
    naming it.  No host read: capturable.  There is no CPU path (``bounds.posed_vertices_torch`` is the torch form)."""
    who = "posed_vertices_fn"
    no_grad(who, {"params['shapes']": params.get("shapes")}, _WHY)
    V, J, par, dev = body_arrays(who, body, _WHY, "kernels of csrc/frame_bounds.hip", "posed_vertices_torch is the torch form",
                                 check_weights=True)
    flat = frame_params(who, params, ("poses", "shapes", "R", "Th"), J, int(body["shapedirs"].shape[2]), dev)
    return _PosedVertices.apply(flat["poses"], flat["R"], flat["Th"], flat["shapes"], body, V, J, par)


# ---- the targets ----------------------------------------------------------------------------------------------------------------------

class KeypointTargets:
    """What a frame's keypoints are compared with, as static tensors: ``regressor`` (Kp,V) dense, keypoint k = ``regressor[k] @
    world_vertex``; the 2D part ``K`` (C,3,3), ``RT`` (C,3,4) -- the pair ``bounds.bound_masks`` takes (``bounds.camera_KRT``) --
    ``uv`` (C,Kp,2) in pixels and ``conf`` (C,Kp) >= 0; the 3D part ``xyz`` (Kp,3) and ``conf3`` (Kp).  Either part may be absent (all
    of its tensors ``None``), not both.  ``sigma`` (pixels) / ``sigma3`` (metres): the Geman-McClure scale, ``<= 0`` for plain squares;
    ``weight2d`` / ``weight3d``: the terms' weights.  Float32, contiguous, on one device, none requiring grad; Kp = 1..128.

    ``copy_(other)`` loads new values of the same shapes (a captured step reads them at replay; the four scalars are launch
    arguments: a capture keeps the ones it was made with).  After a call of :func:`keypoint_loss`, ``flags`` (C) int32 has bit 0 set
    for a camera with a keypoint at ``uvw_z <= 0`` (such an entry adds nothing), and ``keypoints`` (Kp,3) holds the regressed points."""

    TENSORS = ("regressor", "K", "RT", "uv", "conf", "xyz", "conf3")
    SCALARS = ("sigma", "sigma3", "weight2d", "weight3d")

    def __init__(self, regressor, K=None, RT=None, uv=None, conf=None, xyz=None, conf3=None, sigma=0.0, sigma3=0.0, weight2d=1.0,
                 weight3d=1.0):
        who = "KeypointTargets"
        if not isinstance(regressor, torch.Tensor) or regressor.dim() != 2:
            raise ValueError(f"{who}: regressor must be a (Kp, V) tensor")
        Kp, V = int(regressor.shape[0]), int(regressor.shape[1])
        if not 1 <= Kp <= KEYPOINTS_MAX:
            raise ValueError(f"{who}: Kp = {Kp} keypoints (the rows of regressor); the kernels take 1..{KEYPOINTS_MAX}")
        if V < 1:
            raise ValueError(f"{who}: regressor must have V >= 1 columns")
        part2d, part3d = {"K": K, "RT": RT, "uv": uv, "conf": conf}, {"xyz": xyz, "conf3": conf3}
        has2d, has3d = any(t is not None for t in part2d.values()), any(t is not None for t in part3d.values())
        if not has2d and not has3d:
            raise ValueError(f"{who}: neither the 2D part (K, RT, uv, conf) nor the 3D part (xyz, conf3) is present")
        for part, present in ((part2d, has2d), (part3d, has3d)):
            missing = [k for k, t in part.items() if t is None]
            if present and missing:
                raise ValueError(f"{who}: {', '.join(missing)} missing: a part is given whole ({', '.join(part)}) or not at all")
        if has2d and (not isinstance(K, torch.Tensor) or K.dim() != 3 or K.shape[0] < 1):
            raise ValueError(f"{who}: K must be a (C,3,3) tensor with C >= 1")
        C = int(K.shape[0]) if has2d else 0
        dev = regressor.device
        shapes = {"regressor": (Kp, V), "K": (C, 3, 3), "RT": (C, 3, 4), "uv": (C, Kp, 2), "conf": (C, Kp), "xyz": (Kp, 3), "conf3": (Kp,)}
        given = {"regressor": regressor, **part2d, **part3d}
        no_grad(who, given, _WHY_TARGET)
        for name, t in given.items():
            if t is not None:
                need(who, t, name, shapes[name], device=dev)
            setattr(self, name, t)
        self.sigma, self.sigma3, self.weight2d, self.weight3d = float(sigma), float(sigma3), float(weight2d), float(weight3d)
        self.Kp, self.V, self.C, self.has3d, self.device = Kp, V, C, has3d, dev
        self.flags = torch.zeros(C, dtype=torch.int32, device=dev)
        self.keypoints = torch.zeros((Kp, 3), dtype=torch.float32, device=dev)

    @property
    def key(self):
        """What a captured step bakes in: the sizes, which parts are present, and the four scalars."""
        return (self.C, self.Kp, self.V, self.C > 0, self.has3d) + tuple(getattr(self, k) for k in self.SCALARS)

    def clone(self):
        """Targets of the same values on tensors of their own."""
        c = lambda t: None if t is None else t.detach().clone()                      # noqa: E731
        return KeypointTargets(*(c(getattr(self, k)) for k in self.TENSORS), **{k: getattr(self, k) for k in self.SCALARS})

    def copy_(self, other):
        if not isinstance(other, KeypointTargets):
            raise ValueError("KeypointTargets.copy_: other must be a KeypointTargets")
        for name in self.TENSORS:
            dst, src = getattr(self, name), getattr(other, name)
            if (dst is None) != (src is None) or (dst is not None and dst.shape != src.shape):
                raise ValueError(f"KeypointTargets.copy_: {name} must be {'absent' if dst is None else f'of shape {tuple(dst.shape)}'}, "
                                 f"got {'none' if src is None else tuple(src.shape)}")
        with torch.no_grad():
            for name in self.TENSORS:
                if getattr(self, name) is not None and getattr(self, name) is not getattr(other, name):
                    getattr(self, name).copy_(getattr(other, name))
        for name in self.SCALARS:
            setattr(self, name, getattr(other, name))
        return self


# ---- the loss -------------------------------------------------------------------------------------------------------------------------

class _KeypointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world_vertex, tg):
        from ._lib import KeypointLossArgs, call, lib, ptr
        dev = world_vertex.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty_like(world_vertex)
        ws = torch.empty(int(lib().moss_keypoint_loss_workspace_bytes(tg.C, tg.Kp)), dtype=torch.uint8, device=dev)
        a = KeypointLossArgs()
        a.V, a.Kp, a.C = tg.V, tg.Kp, tg.C
        a.world_vertex, a.regressor = world_vertex.data_ptr(), tg.regressor.data_ptr()
        a.K, a.RT, a.uv, a.conf, a.xyz, a.conf3 = (ptr(getattr(tg, k)) for k in ("K", "RT", "uv", "conf", "xyz", "conf3"))
        a.sigma, a.sigma3, a.weight2d, a.weight3d = tg.sigma, tg.sigma3, tg.weight2d, tg.weight3d
        a.loss, a.g_world_vertex, a.keypoints = loss.data_ptr(), g.data_ptr(), tg.keypoints.data_ptr()
        a.flags = tg.flags.data_ptr() if tg.C else None
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        call("moss_keypoint_loss", dev, ctypes.byref(a))
        ctx.save_for_backward(g)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return grad_out * g, None


def keypoint_loss(world_vertex, targets):
    """The scalar keypoint loss of ``world_vertex`` (V,3) against ``targets`` (a :class:`KeypointTargets`) on the device (C ABI
    ``moss_keypoint_loss``, three launches; the formula in include/moss_raster.h):

        X_k = regressor[k] @ world_vertex,   u = the projection of X_k by K_c, RT_c,   rho_s(r2) = s^2 r2 / (s^2 + r2)
        loss = weight2d / (C Kp) sum_c sum_k conf rho_sigma(|u - uv|^2)  +  weight3d / Kp sum_k conf3 rho_sigma3(|X_k - xyz_k|^2)

    The call forms the value and its gradient to ``world_vertex`` together; the backward returns ``grad_out`` times that gradient.
    ``world_vertex``: float32, contiguous, on the targets' GPU (it may require grad).  ``targets.flags`` and ``targets.keypoints``
    are written by the call.  No host read: capturable.  There is no CPU path (:func:`keypoint_loss_torch` is the torch form)."""
    who = "keypoint_loss"
    if not isinstance(targets, KeypointTargets):
        raise ValueError(f"{who}: targets must be a KeypointTargets")
    need_gpu(who, targets.device, "kernels of csrc/keypoints.hip", "keypoint_loss_torch is the torch form")
    need(who, world_vertex, "world_vertex", (targets.V, 3), device=targets.device)
    return _KeypointLoss.apply(world_vertex, targets)


def project_torch(X, K, RT):
    """``(u (C,N,2), z (C,N))`` of points ``X`` (N,3) seen by ``K`` (C,3,3) / ``RT`` (C,3,4): ``cam = RT [X, 1]``, ``uvw = K cam``,
    ``u = uvw[:2] / uvw[2]``, ``z = uvw[2]`` -- the convention of ``bounds.project_corners_numpy``.  Where ``z <= 0``, ``u`` is ``uvw[:2]``."""
    cam = torch.einsum("crq,nq->cnr", RT[:, :, :3], X) + RT[:, None, :, 3]
    uvw = torch.einsum("crq,cnq->cnr", K, cam)
    z = uvw[..., 2]
    return uvw[..., :2] / torch.where(z <= 0, torch.ones_like(z), z)[..., None], z


def _rho(r2, sigma):
    return r2 if sigma <= 0 else (sigma * sigma) * r2 / (sigma * sigma + r2)


def keypoint_loss_torch(world_vertex, targets):
    """:func:`keypoint_loss`'s contract in torch ops, in the dtype and on the device of ``world_vertex`` (the targets' tensors are
    converted to them): differentiable with respect to ``world_vertex``; ``targets.flags`` is written.  The float64 yardstick of the
    tests and the float32 stand-in of scripts/keypoint_fit_times.py; it is not a fallback."""
    tg = targets
    as_wv = lambda t: t.to(world_vertex)                                              # noqa: E731
    X = as_wv(tg.regressor) @ world_vertex
    loss = world_vertex.new_zeros(())
    if tg.C:
        u, z = project_torch(X, as_wv(tg.K), as_wv(tg.RT))
        behind = z <= 0
        r2 = ((u - as_wv(tg.uv)) ** 2).sum(-1)
        term = torch.where(behind, torch.zeros_like(r2), as_wv(tg.conf) * _rho(r2, tg.sigma))
        loss = loss + tg.weight2d / (tg.C * tg.Kp) * term.sum()
        with torch.no_grad():
            tg.flags.copy_(behind.any(1))
    if tg.has3d:
        r2 = ((X - as_wv(tg.xyz)) ** 2).sum(-1)
        loss = loss + tg.weight3d / tg.Kp * (as_wv(tg.conf3) * _rho(r2, tg.sigma3)).sum()
    return loss
