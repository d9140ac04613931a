"""Fitting a frame's SMPL parameters to images through a frozen avatar: the gradients of MOSS's deformation chain to ``poses``, ``R``
and ``Th`` as HIP ops, and a small fit loop on top.

The training step treats a frame's pose as data (``lbs.smpl_frame_fused`` refuses a ``poses`` that requires grad, ``lbs.lbs_deform``
an ``R`` or ``Th``).  Driving a trained avatar from footage without SMPL fits, or cleaning up the fits a dataset ships, needs the
opposite: the avatar is data and the frame's parameters are the variables.

* :func:`posed_frame` -- one ``autograd.Function``: forward = ``moss_smpl_frame_forward`` + ``moss_lbs_deform_forward`` (what
  ``coarse_deform_c2source(fused_frame=True)`` runs), backward = ``moss_lbs_deform_backward_frame`` + ``moss_smpl_frame_backward_pose``
  (include/moss_raster.h; csrc/lbs.hip, csrc/smpl_frame.hip): three launches forward and six backward, float64 sums in a fixed order, bitwise reproducible,
  capturable.  Gradients flow to ``params['poses']``, ``params['R']`` and ``params['Th']`` and to nothing else.
* :func:`posed_frame_torch` -- the same contract composed from the differentiable torch forms of ``moss_amd.lbs`` (any dtype or
  device): the float64 yardstick of the tests and the float32 stand-in of scripts/pose_fit_times.py.  It is not a fallback;
  :func:`posed_frame` has no CPU path.
* :class:`PoseFitter` -- ``fit(cameras, gt_images, regions, smpl_param, steps)``: render through the rasterizer with ``transforms`` /
  ``translation`` in the op, MOSS's photometric loss on the view's region, one AdamW launch per step; eager or replayed from a hipGraph.
  ``fit(..., keypoints=, photometric=)`` adds or substitutes the keypoint term of ``moss_amd.keypoints``.

What is differentiated: the Rodrigues of ``poses``, the kinematic chain, the pose blend shapes' offsets gathered at the Gaussians'
vertices, the blend of ``A_obs``, ``R`` and ``Th``.  What is held fixed: ``shapes``, the body model, the big pose, the Gaussians, and --
a modelling decision -- the outputs of the pose head and of the LBS-weight network: they are re-evaluated on the current ``poses`` in
every step, but enter the deformation as data (no gradient goes through the two networks to ``poses``).

Everything here imports without a GPU.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from ._checks import body_arrays, frame_params, need, need_ids, no_grad
from .lbs import (_launch_lbs_backward, _launch_lbs_forward, _launch_smpl_frame_backward, _launch_smpl_frame_forward, batch_rodrigues,
                  deform_torch, smpl_joint_transforms, vertex_offsets)

__all__ = ["posed_frame", "posed_frame_torch", "PoseFitter", "rotation_to_axis_angle"]


# ---- the op ---------------------------------------------------------------------------------------------------------------------------

class _PosedFrame(torch.autograd.Function):
    """``lbs._SmplFrame`` followed by ``lbs._LbsDeform`` in one node, with the backwards that also form ``g_poses``, ``g_R``, ``g_Th``."""

    @staticmethod
    def forward(ctx, poses, R, Th, par, vt, sd, pd, jr, W, poses_big, shapes_big, shapes, ids, x, L, cR):
        A_big, A_obs, d, _, saved = _launch_smpl_frame_forward(cR, par, vt, sd, pd, jr, poses_big, shapes_big, poses, shapes, ids,
                                                               want_saved=True)
        T, t, p, _ = _launch_lbs_forward(ids, W, L, A_big, A_obs, d, R, Th, x, want_weights=False)
        ctx.set_materialize_grads(False)                        # (no zero-fill launches for the cotangents nobody formed)
        ctx.save_for_backward(poses, R, Th, pd, W, ids, x, L, cR, A_big, A_obs, d, saved)
        ctx.par, ctx.V, ctx.has_L, ctx.has_cR = par, int(vt.shape[0]), L is not None, cR is not None
        return T, t, p

    @staticmethod
    def backward(ctx, gT, gt, gp):
        poses, R, Th, pd, W, ids, x, L, cR, A_big, A_obs, d, saved = ctx.saved_tensors
        L = L if ctx.has_L else None
        cR = cR if ctx.has_cR else None
        g = _launch_lbs_backward([ids, W, L, A_big, A_obs, d, R, Th, x], gT, gt, gp, ("g_A_obs", "g_d", "g_R", "g_Th"))
        gA, gd = (g["g_A_obs"], g["g_d"]) if int(ids.shape[0]) > 0 else (None, None)     # (P = 0: g_A_obs is not written, and is zero)
        gposes = _launch_smpl_frame_backward(ctx.par, ctx.V, pd, ids, saved, gA, gd, poses=poses, cR=cR)
        return (gposes.reshape(poses.shape), g["g_R"], g["g_Th"]) + (None,) * 13


def posed_frame(body, W, params, t_params, vert_ids, x, lbs_offsets=None, correct_Rs=None):
    """A frame's per-Gaussian transforms as a function of the frame's SMPL parameters, on the device:
    ``(T (P,3,3), t (P,3), p (P,3))`` -- MOSS's ``transforms``, ``translation`` and ``world_src_pts``, what
    ``lbs.coarse_deform_c2source(fused_frame=True)`` computes -- with gradients to ``params['poses']``, ``params['R']`` and
    ``params['Th']`` (C ABI ``moss_lbs_deform_backward_frame`` and ``moss_smpl_frame_backward_pose``; formulas in
    include/moss_raster.h).  Two launches forward and three backward for the frame, one forward and three backward for the Gaussians.

    ``body``: ``v_template`` (V,3), ``shapedirs`` (V,3,B), ``posedirs`` (V,3,9(J-1)), ``J_regressor`` (J,V), ``kintree_table`` (2,J);
    ``W`` (V,J) the blend weights; ``params``: ``poses`` (3J elements), ``shapes``, ``R`` (3,3), ``Th`` (3 elements); ``t_params``:
    the big pose's ``poses`` and ``shapes``; ``vert_ids`` (P,) int64; ``x`` (P,3) the canonical positions; ``lbs_offsets`` (P,J) or
    None; ``correct_Rs`` (J-1,3,3) or None.  All float32, contiguous, on one GPU; J = 1..64.

    The avatar is frozen here: ``x``, ``lbs_offsets``, ``correct_Rs``, ``shapes``, ``W``, the big pose and the body model are data,
    and one that requires grad raises ``ValueError`` naming it.  The gradient of ``R`` is that of ``M = R O3`` as the header defines
    the op (the reference writes ``torch.inverse(R)`` of the transpose; the two agree on rotations).  A Gaussian with an id outside
    [0, V) gives NaN rows and adds nothing to the three gradients.  There is no CPU path (:func:`posed_frame_torch` is the torch form)."""
    who = "posed_frame"
    why = "it is data of the fit (the avatar is frozen: gradients go to params['poses'], params['R'] and params['Th'] only)"
    no_grad(who, {"params['shapes']": params.get("shapes"), "t_params['poses']": t_params.get("poses"),
                  "t_params['shapes']": t_params.get("shapes"), "x": x, "lbs_offsets": lbs_offsets, "correct_Rs": correct_Rs}, why)
    V, J, par, dev = body_arrays(who, body, why, "deformation kernels", "posed_frame_torch is the torch form", weights=W)
    B = int(body["shapedirs"].shape[2])
    big = frame_params(who, t_params, ("poses", "shapes"), J, B, dev, name="t_params")
    frame = frame_params(who, params, ("poses", "shapes", "R", "Th"), J, B, dev)
    P = int(need_ids(who, vert_ids, dev).shape[0])
    for name, t, shape in (("x", x, (P, 3)), ("lbs_offsets", lbs_offsets, (P, J)), ("correct_Rs", correct_Rs, (J - 1, 3, 3))):
        if t is not None or name == "x":
            need(who, t, name, shape, device=dev)
    return _PosedFrame.apply(frame["poses"], frame["R"].reshape(3, 3), frame["Th"], par, body["v_template"], body["shapedirs"],
                             body["posedirs"], body["J_regressor"], W, big["poses"], big["shapes"], frame["shapes"], vert_ids, x,
                             lbs_offsets, correct_Rs)


def posed_frame_torch(body, W, params, t_params, vert_ids, x, lbs_offsets=None, correct_Rs=None):
    """:func:`posed_frame`'s contract composed from the differentiable torch forms of ``moss_amd.lbs`` --
    ``batch_rodrigues``, ``smpl_joint_transforms``, ``vertex_offsets``, ``deform_torch`` -- in the inputs' dtype and on their device:
    ``(T, t, p)``, differentiable with respect to whatever requires grad.  The float64 yardstick of the tests and the float32 stand-in
    of scripts/pose_fit_times.py; it is not a fallback."""
    J = W.shape[-1]
    vt = body["v_template"]
    body = {**body, "weights": W}
    A_big = smpl_joint_transforms(body, {"R": None, "Th": None, **t_params})[0][0]       # (the big pose's R and Th are not read)
    rot = batch_rodrigues(params["poses"].reshape(-1, 3).to(vt)).reshape(J, 3, 3)
    if correct_Rs is not None:
        rot = torch.cat([rot[:1], rot[1:] @ correct_Rs.reshape(J - 1, 3, 3)], 0)
    A_obs = smpl_joint_transforms(body, params, rot_mats=rot)[0][0]
    D = vertex_offsets(body, params, t_params, rot)
    T, t, p, _ = deform_torch(vert_ids, W, lbs_offsets, A_big, A_obs, D[vert_ids], params["R"].reshape(3, 3), params["Th"].reshape(3), x=x)
    return T, t, p


def rotation_to_axis_angle(R):
    """(3,3) rotation -> (3,) axis-angle (the inverse of ``batch_rodrigues`` away from angle pi), in torch, on R's device."""
    R = R.reshape(3, 3)
    w = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * w.norm()                                          # sin(angle)
    c = 0.5 * (R.diagonal().sum() - 1.0)                        # cos(angle)
    angle = torch.atan2(s, c)
    scale = torch.where(s > 1e-6, angle / (2.0 * s).clamp_min(1e-12), torch.full_like(s, 0.5))
    return scale * w


# ---- the fit loop ---------------------------------------------------------------------------------------------------------------------

class PoseFitter:
    """``fitter = PoseFitter(pc, view, bg)``; ``fitted, losses = fitter.fit(cameras, gt_images, regions, smpl_param, steps)`` fits one
    frame's ``poses`` (3J), ``Th`` (3) and, with ``fit_R``, ``Rh`` (3; ``R = batch_rodrigues(Rh)`` in torch, so ``R`` stays a rotation)
    to images of that frame, through a frozen avatar.

    ``pc``, ``view``, ``bg``: what ``MossPlayer`` takes -- a ``GaussianSet`` with ``SMPL_NEUTRAL`` and ``knn`` (and, with
    ``motion_offset_flag``, ``auto_regression`` and ``cross_attention_lbs``); a camera with ``big_pose_smpl_param`` and
    ``big_pose_world_vertex``.  The fitter owns no model parameter and never writes one (nor a ``.grad`` of one: the rasterizer sees
    detached views).  ``template_index`` / ``lbs_weights_precision``: as in ``MossPlayer``.

    One step: for a model with ``motion_offset_flag`` the pose head (``pose_head_fused``) and the LBS-weight network
    (``cross_attention_lbs_fused``) are re-run on the current ``poses`` under ``no_grad`` and their outputs enter
    :func:`posed_frame` as data -- NO gradient goes through the two networks to ``poses``: a modelling decision (the networks refine
    a pose, they are not the parameterisation being fitted).  Then :func:`posed_frame`, one ``render()`` per camera with
    ``transforms`` / ``translation`` inside the op (``RAW_POSE``; the cameras' gradients are summed), the loss
    (``loss.training_loss_moss_fused`` on the view's region, ``training_loss_fused`` without one; ``loss=`` overrides it with a
    callable ``(image, alpha, gt_image, bkgd_mask, region) -> scalar``), the backward, and ``optim.AdamW`` (``weight_decay=0``): one
    launch for the leaves.

    ``fit(..., keypoints=targets)`` adds ``keypoints.keypoint_loss(keypoints.posed_vertices_fn(body, params), targets)`` of the RAW
    ``poses``, ``R`` and ``Th`` to the loss (the vertices ``player.frame``'s region uses and a detector saw: the refined rotations
    and the LBS offsets do not enter it); ``photometric=False`` leaves that term alone -- no networks, no ``posed_frame``, no render:
    the initialisation from far away, where the photometric term has no overlap to descend on.

    ``capture=True``: everything of the step but the update is a ``GraphedStep``; a replay followed by the (eager, one-launch) update
    equals the eager step bit for bit (``optim.AdamW`` takes its step count as a launch argument, so it stays outside the graph).  A
    new target, camera or start is loaded by ``copy_`` into static tensors; other intrinsics or another number of cameras capture again.

    ``lr``: one rate or ``{"poses", "Th", "Rh"}``.  ``fit`` returns ``({"poses" (1,3J), "Rh" (3,), "R" (3,3), "Th" (1,3)}, losses
    (steps,))``: the loss BEFORE each update, one device tensor; nothing is read on the host inside the loop, and ``fit`` ends with one
    check of the rasterizer's status (it synchronises)."""

    _frame_fn = staticmethod(posed_frame)                       # (scripts/pose_fit_times.py times the step with posed_frame_torch here)

    def __init__(self, pc, view, bg, lr=2e-3, fit_R=True, capture=False, lbs_weights_precision="f32", template_index=False, loss=None,
                 lambda_dssim=0.2, lambda_mask=0.5):
        from .lbs_weights import PRECISIONS
        self.motion = bool(getattr(pc, "motion_offset_flag", False))
        needs = ("SMPL_NEUTRAL", "knn") + (("auto_regression", "cross_attention_lbs") if self.motion else ())
        missing = [a for a in needs if not hasattr(pc, a)]
        if missing:
            raise ValueError(f"PoseFitter: the model lacks {missing}")
        for a in ("big_pose_smpl_param", "big_pose_world_vertex"):
            if not hasattr(view, a):
                raise ValueError(f"PoseFitter: the view has no {a}")
        if lbs_weights_precision not in PRECISIONS:
            raise ValueError(f"PoseFitter: lbs_weights_precision must be one of {PRECISIONS}, got {lbs_weights_precision!r}")
        dev = pc._xyz.device
        if dev.type != "cuda":
            raise ValueError("PoseFitter runs the HIP deformation kernels and the rasterizer: the model must be on a GPU")
        self.pc, self.view, self.bg = pc, view, bg
        self.device = dev
        self.fit_R, self.capture = bool(fit_R), bool(capture)
        self.lbs_weights_precision = lbs_weights_precision
        self.loss_fn, self.lambda_dssim, self.lambda_mask = loss, float(lambda_dssim), float(lambda_mask)
        body = pc.SMPL_NEUTRAL
        self.J = J = int(body["weights"].shape[-1])
        c32 = lambda t: t.detach().float().contiguous()                                  # noqa: E731
        self.body = {k: (c32(v) if v.is_floating_point() else v) for k, v in body.items() if isinstance(v, torch.Tensor)}
        self.body["kintree_table"] = body["kintree_table"]       # (the table itself: lbs caches its parent list by identity)
        self.big = {k: c32(view.big_pose_smpl_param[k]) for k in ("poses", "shapes")}
        f32 = dict(dtype=torch.float32, device=dev)
        # the leaves and the frame's data, static: a fit loads a start by copy_
        self.poses = torch.zeros(3 * J, **f32).requires_grad_(True)
        self.Th = torch.zeros(3, **f32).requires_grad_(True)
        self.Rh = torch.zeros(3, **f32).requires_grad_(self.fit_R)
        self.R = torch.eye(3, **f32)                             # (read when fit_R is off)
        self.shapes = torch.zeros(int(self.big["shapes"].numel()), **f32)
        self.pose_rotmats = torch.zeros(max(J - 1, 0), 3, 3, **f32)   # (the pose head's NLL target; the NLL is not part of the fit)
        self._leaves = [self.poses, self.Th] + ([self.Rh] if self.fit_R else [])
        for p in self._leaves:
            p.grad = torch.zeros_like(p)
        rates = lr if isinstance(lr, dict) else {"poses": lr, "Th": lr, "Rh": lr}
        from .optim import AdamW
        groups = [{"params": [self.poses], "lr": float(rates["poses"])}, {"params": [self.Th], "lr": float(rates["Th"])}]
        if self.fit_R:
            groups.append({"params": [self.Rh], "lr": float(rates["Rh"])})
        self.optimizer = AdamW(groups, lr=float(rates["poses"]), weight_decay=0.0)
        with torch.no_grad():
            x = pc.get_xyz.detach().float().contiguous()
            if template_index:
                from .knn_cuda import TemplateIndex
                self.vert_ids = TemplateIndex(view.big_pose_world_vertex).query(x).contiguous()
            else:
                _, ids = pc.knn(view.big_pose_world_vertex[None].float(), x[None])
                self.vert_ids = ids.reshape(-1).contiguous()
        self._views = []                                         # per camera: SimpleNamespace(camera, context, pipe, gt, mask, region, has_mask)
        self._kp = None                                          # the fit's static KeypointTargets, or None
        self._photometric = True
        self._key = None
        self._graphed = None
        self.captures = 0

    # ---- static inputs ----------------------------------------------------------------------------------------------------------------
    def _load_views(self, cameras, gt_images, regions, keypoints=None, photometric=True):
        from .gaussian_renderer import intrinsics_of, static_view
        from .loss import ViewRegion
        key = tuple(intrinsics_of(c) for c in cameras) + tuple(r is not None for r in regions) \
            + tuple(isinstance(g, (tuple, list)) for g in gt_images)
        if keypoints is not None or not photometric:             # (C, Kp, V, has 2D, has 3D, the four scalars), photometric
            key += (None if keypoints is None else keypoints.key, photometric)
        if key != self._key:
            if self._graphed is not None:
                torch.cuda.synchronize(self.device)
            self._graphed, self._views, self._key = None, [], key
            self._kp, self._photometric = None if keypoints is None else keypoints.clone(), photometric
            for cam, region in zip(cameras, regions):
                H, W = intrinsics_of(cam)[:2]
                camera, cx, pipe = static_view(intrinsics_of(cam), {k: torch.empty_like(getattr(cam, k)) for k in
                                                                    ("world_view_transform", "full_proj_transform", "camera_center")})
                static_region = None
                if region is not None:
                    static_region = ViewRegion.from_device(torch.empty_like(region.bound), torch.empty_like(region.rect))
                self._views.append(SimpleNamespace(
                    camera=camera, context=cx, pipe=pipe, region=static_region,
                    gt=torch.empty((3, H, W), dtype=torch.float32, device=self.device),
                    mask=torch.ones((1, H, W), dtype=torch.float32, device=self.device), has_mask=False))
        with torch.no_grad():
            for v, cam, gt, region in zip(self._views, cameras, gt_images, regions):
                for k in ("world_view_transform", "full_proj_transform", "camera_center"):
                    getattr(v.camera, k).copy_(getattr(cam, k))
                image, mask = gt if isinstance(gt, (tuple, list)) else (gt, None)
                v.gt.copy_(image.reshape(v.gt.shape))
                v.has_mask = mask is not None
                if mask is not None:
                    v.mask.copy_(mask.reshape(v.mask.shape))
                if region is not None:
                    v.region.copy_(region)
        if keypoints is not None:
            self._kp.copy_(keypoints)

    def _load_start(self, smpl_param):
        J = self.J
        with torch.no_grad():
            self.poses.copy_(smpl_param["poses"].reshape(-1))
            self.Th.copy_(smpl_param["Th"].reshape(-1))
            self.shapes.copy_(smpl_param["shapes"].reshape(-1))
            R = smpl_param["R"].reshape(3, 3).float()
            self.R.copy_(R)
            if self.fit_R:
                self.Rh.copy_(smpl_param["Rh"].reshape(-1) if "Rh" in smpl_param else rotation_to_axis_angle(R))
            if J > 1:
                target = smpl_param.get("pose_rotmats")
                self.pose_rotmats.copy_(batch_rodrigues(self.poses.reshape(J, 3))[1:] if target is None else target.reshape(J - 1, 3, 3))
            for p in self._leaves:                               # a fit starts the optimizer afresh
                st = self.optimizer.state[p]
                if len(st):
                    st["step"] = 0
                    st["exp_avg"].zero_()
                    st["exp_avg_sq"].zero_()

    # ---- one step ----------------------------------------------------------------------------------------------------------------------
    def _frozen_model(self):
        """What ``render()`` reads of the model, detached: the rasterizer's backward then forms no gradient for a model parameter."""
        pc = self.pc
        return SimpleNamespace(get_xyz=pc.get_xyz.detach(), get_features=pc.get_features.detach(), _opacity=pc._opacity.detach(),
                               _scaling=pc._scaling.detach(), _rotation=pc._rotation.detach(), active_sh_degree=pc.active_sh_degree,
                               max_sh_degree=pc.max_sh_degree, spatially_ordered=getattr(pc, "spatially_ordered", False))

    def _view_loss(self, v, out):
        from .loss import training_loss_fused, training_loss_moss_fused
        image, alpha = out["render"], out["render_alpha"]
        if self.loss_fn is not None:
            return self.loss_fn(image, alpha, v.gt, v.mask, v.region)
        lambda_mask = self.lambda_mask if v.has_mask else 0.0
        if v.region is not None:
            return training_loss_moss_fused(image, alpha, v.gt, v.mask, v.region, lambda_dssim=self.lambda_dssim, lambda_mask=lambda_mask)
        return training_loss_fused(image, alpha, v.gt, v.mask, lambda_dssim=self.lambda_dssim, lambda_mask=lambda_mask)

    def _compute(self):
        """The loss of the static inputs and its gradients into the leaves' static ``.grad`` tensors; returns the detached loss."""
        if not self._photometric:
            return self._compute_keypoints_only()
        from .gaussian_renderer import render
        pc, J = self.pc, self.J
        frozen = self._frozen_model()
        x = frozen.get_xyz
        if not x.is_contiguous() or x.dtype != torch.float32:
            x = x.float().contiguous()
        L = Rs = None
        with torch.no_grad():
            if self.motion:
                from .lbs_weights import cross_attention_lbs_fused
                from .pose import pose_head_fused
                Rs = pose_head_fused(pc.auto_regression, self.poses.detach(), self.pose_rotmats)["Rs"].detach().reshape(J - 1, 3, 3)
                L = cross_attention_lbs_fused(pc.cross_attention_lbs, x[None], Rs, precision=self.lbs_weights_precision)
                L = L.detach().reshape(x.shape[0], J)
        R = batch_rodrigues(self.Rh[None])[0] if self.fit_R else self.R
        params = {"poses": self.poses, "shapes": self.shapes, "R": R.contiguous(), "Th": self.Th}
        T, t, _ = self._frame_fn(self.body, self.body["weights"], params, self.big, self.vert_ids, x, lbs_offsets=L, correct_Rs=Rs)
        loss = None
        for v in self._views:
            out = render(v.camera, frozen, v.pipe, self.bg, transforms=T, translation=t)
            term = self._view_loss(v, out)
            loss = term if loss is None else loss + term
        if self._kp is not None:
            loss = loss + self._keypoint_term(params)
        for p in self._leaves:
            p.grad.zero_()
        loss.backward()
        return loss.detach()

    def _keypoint_term(self, params):
        """The keypoint loss of the RAW ``poses``, ``R`` and ``Th`` (what ``player.frame``'s region uses and what a detector saw: the
        refined rotations and the LBS offsets do not enter)."""
        from .keypoints import keypoint_loss, posed_vertices_fn
        return keypoint_loss(posed_vertices_fn(self.body, params), self._kp)

    def _compute_keypoints_only(self):
        """``_compute`` without the photometric term: no networks, no ``posed_frame``, no render."""
        R = batch_rodrigues(self.Rh[None])[0] if self.fit_R else self.R
        loss = self._keypoint_term({"poses": self.poses, "shapes": self.shapes, "R": R.contiguous(), "Th": self.Th})
        for p in self._leaves:
            p.grad.zero_()
        loss.backward()
        return loss.detach()

    def step(self):
        """One step on what the last ``fit`` loaded (a replay when captured), then the update; returns the loss before the update, a
        device scalar that the next step overwrites when captured."""
        loss = self._graphed() if self._graphed is not None else self._compute()
        self.optimizer.step()
        return loss

    def fit(self, cameras, gt_images, regions, smpl_param, steps, keypoints=None, photometric=True):
        """Fit the frame seen by ``cameras`` (one camera or a list of cameras of the same frame) to ``gt_images`` (per camera a
        (3,H,W) image, or an ``(image, bkgd_mask)`` pair: without a mask the loss has no alpha term) on ``regions`` (per camera a
        ``loss.ViewRegion`` or None), starting from ``smpl_param`` (``poses``, ``shapes``, ``R``, ``Th``; ``Rh`` if it has one, else
        the axis-angle of ``R``), for ``steps`` steps.  See the class for what comes back.

        ``keypoints``: a ``keypoints.KeypointTargets`` on the model's GPU over the body's V vertices; the step then adds
        ``keypoint_loss(posed_vertices_fn(body, params), keypoints)`` of the raw ``poses``, ``R`` and ``Th`` to the loss (its cameras
        are the targets' own ``K`` / ``RT``).  ``photometric=False`` (needs ``keypoints``): the step is that term alone -- no networks,
        no ``posed_frame``, no render; ``cameras``, ``gt_images`` and ``regions`` may be None: the initialisation from far away.  New
        targets of the same sizes are loaded by ``copy_``; other sizes, parts or scalars capture again."""
        photometric = bool(photometric)
        if keypoints is not None:
            from .keypoints import KeypointTargets
            V = int(self.body["v_template"].shape[0])
            if not isinstance(keypoints, KeypointTargets) or keypoints.device != self.device or keypoints.V != V:
                raise ValueError(f"PoseFitter.fit: keypoints must be a KeypointTargets on {self.device} over the body's V = {V} vertices")
        elif not photometric:
            raise ValueError("PoseFitter.fit: photometric=False leaves no loss without keypoints")
        if not photometric:
            cameras, gt_images, regions = [], [], []
        single = not isinstance(cameras, (list, tuple))
        cameras = [cameras] if single else list(cameras)
        n = len(cameras)
        if single:
            gt_images, regions = [gt_images], [regions]
        gt_images = list(gt_images)
        regions = [None] * n if regions is None else list(regions)
        if (n == 0 and photometric) or len(gt_images) != n or len(regions) != n:
            raise ValueError("PoseFitter.fit: one ground truth and one region (or None) per camera")
        steps = int(steps)
        self._load_views(cameras, gt_images, regions, keypoints, photometric)
        self._load_start(smpl_param)
        losses = torch.zeros(max(steps, 0), dtype=torch.float32, device=self.device)
        if self.capture and self._graphed is None and steps > 0:
            from .graphs import GraphedStep
            self._compute()                                      # (eager first: the synchronous forwards size the binning capacities)
            if self._views:
                context = self._views[0].context
            else:                                                # (no render is captured: a context of its own keeps the default one untouched)
                from .diff_gaussian_rasterization._C import RasterContext
                context = RasterContext()
            self._graphed = GraphedStep(self._compute, warmup=2, device=self.device, context=context,
                                        extra_contexts=[v.context for v in self._views[1:]])
            self.captures += 1
        for k in range(steps):
            losses[k].copy_(self.step())
        from .diff_gaussian_rasterization._C import CapacityOverflow
        for v in self._views:
            try:
                v.context.check_status()
            except CapacityOverflow as e:
                raise RuntimeError("PoseFitter.fit: a view overflowed the rasterizer's binning capacity and rendered nothing in a step "
                                   "(the capacity has been grown: fit again)") from e
        with torch.no_grad():
            R = batch_rodrigues(self.Rh.detach()[None])[0] if self.fit_R else self.R
            fitted = {"poses": self.poses.detach().clone().reshape(1, -1), "Rh": self.Rh.detach().clone(), "R": R.clone(),
                      "Th": self.Th.detach().clone().reshape(1, 3)}
        return fitted, losses
